"""ROW PRIORS on a host without a GPU (include/mi355rec_diag.h): the playlist request with a prior through the node handle
(served by the product's CPU backend, csrc/cpu_backend.cpp) on tests/golden/catalogue4096.npz: the contract, the three
identities, every composition of the family, massive ties, every refusal and the Python keywords.  Expected results come from
tests/prior_oracle.py: equal ids, bit-equal scores, equal counts."""
import ctypes
import inspect

import numpy as np
import pytest

from tests.diverse_oracle import check3
from tests.labels_oracle import check
from tests.playlist_labels_oracle import uniform_labels
from tests.prior_oracle import blended, expected_diverse, expected_prior, prior_kinds, request_call, scores_of


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
N_LABELS = 12
BETAS = (0.25, 1.0, -0.5, 4.0, -4.0, 2.0 ** -20)


@pytest.fixture(scope="module")
def node(engine_lib, golden_dir):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = np.ascontiguousarray(np.load(golden_dir / "catalogue4096.npz")["feats"])
    lab = uniform_labels(feats.shape[0], N_LABELS, 3, unlabelled=0.05)
    groups = (np.arange(feats.shape[0]) % 7).astype(np.int32)
    pri = prior_kinds(np.random.default_rng(11), feats.shape[0])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(lab)
        nd.set_groups(groups)
        yield nd, feats, lab, groups, pri


def _fn(nd):
    return nd._lib.mi355rec_sharded_query_playlist_request


def _call(nd, **kw):
    from spotify_recommender_amd import capi
    rc, ids, sc, mmr, p = request_call(capi, _fn(nd), nd._h, **kw)
    assert rc == capi.OK, nd._lib.mi355rec_sharded_last_error(nd._h)
    return ids, sc, mmr, p


def test_contract_and_compositions(node):
    nd, feats, lab, groups, pri = node
    rng = np.random.default_rng(1)
    rows = [int(r) for r in rng.choice(feats.shape[0], size=5, replace=False)]
    vecs = rng.random((3, 12), dtype=np.float32)
    w3, w5 = [1.0, -0.5, 2.0], [1.0, 1.0, -0.75, 3.0, -0.25]   # dislikes included
    wanted = [1, 4, 4, 9]
    s_v, s_vw, s_r, s_rw = scores_of(feats, vecs), scores_of(feats, vecs, w3), scores_of(feats, feats[rows]), scores_of(feats, feats[rows], w5)
    for kind, p in pri.items():
        nd.set_priors(p)
        for beta in BETAS:
            excl = expected_prior(s_v, p, beta, feats, lab, None, [], 40)[0][::2].tolist() + [0, 1, 2]
            for topn in (1, 10, 1024):
                what = f"{kind} beta {beta} top-{topn}"
                check(_call(nd, members=vecs, topn=topn, prior_weight=beta)[:2], expected_prior(s_v, p, beta, feats, lab, None, [], topn), what)
                check(_call(nd, rows=rows, topn=topn, prior_weight=beta)[:2], expected_prior(s_r, p, beta, feats, lab, None, rows, topn),
                      what + " by row")
                check(_call(nd, members=vecs, weights=w3, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_vw, p, beta, feats, lab, None, [], topn), what + " weights")
                check(_call(nd, members=vecs, exclude=excl, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_v, p, beta, feats, lab, None, excl, topn), what + " exclude")
                check(_call(nd, members=vecs, where=WHERE, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_v, p, beta, feats, lab, None, [], topn, WHERE), what + " filter")
                check(_call(nd, members=vecs, labels=wanted, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_v, p, beta, feats, lab, wanted, [], topn), what + " labels")
                check(_call(nd, rows=rows, weights=w5, exclude=excl, where=WHERE, labels=wanted, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_rw, p, beta, feats, lab, wanted, rows + excl, topn, WHERE), what + " all together")
            # MMR and caps: the pool is the top-`pool` by v and rel = v
            for pool in (40, 1024):
                pl = expected_prior(s_rw, p, beta, feats, lab, wanted, rows + excl, pool, WHERE)
                kw = dict(rows=rows, weights=w5, exclude=excl, where=WHERE, labels=wanted, topn=10, pool=pool, prior_weight=beta)
                for lam in (0.0, 0.5, 1.0):
                    check3(_call(nd, lam=lam, **kw)[:3], expected_diverse(pl, feats, lam, 10), f"{kind} {beta} diverse {pool} {lam}")
                    got = _call(nd, lam=lam, max_per_group=1, **kw)
                    check3(got[:3], expected_diverse(pl, feats, lam, 10, groups, 1), f"{kind} {beta} capped {pool} {lam}")
                    assert got[3] == pl[0].size


def test_identities(node):
    nd, feats, lab, groups, pri = node
    rows, wanted = [7, 900, 4000], [2, 3]
    s = scores_of(feats, feats[rows])
    nd.set_priors(pri["signed"])
    for kw in (dict(rows=rows, topn=50), dict(rows=rows, topn=50, labels=wanted, where=WHERE),
               dict(rows=rows, topn=10, lam=0.5, pool=40, max_per_group=2)):
        plain = _call(nd, **kw)
        for zero in (0.0, -0.0):                                   # the flag with beta = 0 is the call without the flag
            check3(_call(nd, prior_weight=zero, **kw)[:3], plain[:3], f"beta {zero}")
    nd.set_priors(np.zeros(feats.shape[0], np.float32))             # all priors +0.0f is no prior
    for beta in BETAS:
        check(_call(nd, rows=rows, topn=50, prior_weight=beta)[:2], _call(nd, rows=rows, topn=50)[:2], f"zero priors, beta {beta}")
    # None drops, a second call replaces, a failed call leaves the previous priors in place
    nd.set_priors(pri["uniform"])
    want = expected_prior(s, pri["uniform"], 1.0, feats, lab, None, rows, 20)
    check(_call(nd, rows=rows, topn=20, prior_weight=1.0)[:2], want, "set")
    nd.set_priors(pri["skewed"])
    check(_call(nd, rows=rows, topn=20, prior_weight=1.0)[:2], expected_prior(s, pri["skewed"], 1.0, feats, lab, None, rows, 20), "replaced")
    from spotify_recommender_amd import capi
    bad = pri["uniform"].copy()
    bad[17] = np.nan
    with pytest.raises(capi.Mi355Error, match="row 17"):
        nd.set_priors(bad)
    check(_call(nd, rows=rows, topn=20, prior_weight=1.0)[:2], expected_prior(s, pri["skewed"], 1.0, feats, lab, None, rows, 20), "kept")
    nd.set_priors(None)
    assert request_call(capi, _fn(nd), nd._h, rows=rows, topn=20, prior_weight=1.0)[0] == capi.ERR_INVALID_ARG


def test_massive_ties(node):
    """Two-valued and all-equal priors with a weight that swamps the similarity's low bits: whole classes of rows share one v
    and the order inside a class is decided by the row."""
    nd, feats, lab, groups, pri = node
    n = feats.shape[0]
    rows = [3, 33]
    s = scores_of(feats, feats[rows])
    for name, p in (("two-valued", (np.arange(n) % 2).astype(np.float32)), ("all-equal", np.full(n, 0.5, np.float32)),
                    ("all-one", np.ones(n, np.float32))):
        nd.set_priors(p)
        for beta in (4.0, -4.0, 1.0):
            for topn in (10, 1024):
                check(_call(nd, rows=rows, topn=topn, prior_weight=beta)[:2], expected_prior(s, p, beta, feats, lab, None, rows, topn),
                      f"{name} beta {beta} top-{topn}")
    # zero rows against everything score 0: with a constant prior the tie is exact and resolved by row
    z = np.zeros((1, 12), np.float32)
    p = np.full(n, 0.25, np.float32)
    nd.set_priors(p)
    ids, sc, _, _ = _call(nd, members=z, topn=100, prior_weight=2.0)
    assert ids.tolist() == list(range(100)) and np.all(sc == np.float32(0.5))
    v = blended(scores_of(feats, feats[rows]), p, 2.0)
    assert v.dtype == np.float32


def test_refusals(node):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd, feats, lab, groups, pri = node
    n = feats.shape[0]
    v = feats[:2]

    def refused(msg, h=None, **kw):
        h = h or nd
        rc = request_call(capi, _fn(h), h._h, **kw)[0]
        text = h._lib.mi355rec_sharded_last_error(h._h).decode()
        assert rc == capi.ERR_INVALID_ARG and msg in text, (kw.keys(), rc, text)

    def set_refused(msg, p, count=None):
        p = np.ascontiguousarray(p, np.float32)
        rc = nd._lib.mi355rec_sharded_set_priors(nd._h, p.ctypes.data_as(ctypes.c_void_p), p.size if count is None else count)
        text = nd._lib.mi355rec_sharded_last_error(nd._h).decode()
        assert rc == capi.ERR_INVALID_ARG and msg in text, (rc, text)

    with NodeEngine(feats[:100], placement=capi.PLACEMENT_AUTO) as fresh:
        refused("has no priors", h=fresh, members=v, prior_weight=1.0)
        refused("has no priors", h=fresh, members=v, prior_weight=0.0)       # the flag needs priors whatever beta is
        refused("has no priors", h=fresh, rows=[1, 2], lam=0.5, pool=20, prior_weight=1.0)
        assert request_call(capi, _fn(fresh), fresh._h, members=v)[0] == capi.OK   # without the flag none are needed
    nd.set_priors(pri["uniform"])
    set_refused("priors for a catalogue of", pri["uniform"][: n - 1])
    set_refused("priors for a catalogue of", np.zeros(n + 1, np.float32))
    for bad, row in ((np.nan, 5), (np.inf, 0), (-np.inf, n - 1), (1.5, 77), (-1.0000001, 78)):
        p = pri["uniform"].copy()
        p[row] = bad
        p[min(row + 9, n - 1)] = bad                                          # the FIRST bad row is named
        set_refused(f"row {row}:", p)
    nd.set_priors(np.where(np.arange(n) % 2 == 0, np.float32(1.0), np.float32(-1.0)))   # +-1 are accepted
    nd.set_priors(pri["uniform"])
    for beta in (float("nan"), float("inf"), 5.0, -4.5):
        refused("prior_weight", members=v, prior_weight=beta)
    assert request_call(capi, _fn(nd), nd._h, members=v, prior_weight=4.0)[0] == capi.OK
    assert request_call(capi, _fn(nd), nd._h, members=v, prior_weight=-4.0)[0] == capi.OK
    assert capi.PlaylistQuery.prior_weight.offset == 84 and ctypes.sizeof(capi.PlaylistQuery) == 88
    refused("MI355REC_PQ_PRIOR in a playlist query of size 84", members=v, prior_weight=1.0, size=84)
    refused("unknown flags", members=v, flags=8)
    refused("unknown flags", members=v, flags=capi.PQ_PRIOR | 16)
    # without the flag the field is never read: garbage in it changes nothing, and the older struct size is still accepted
    q_plain = request_call(capi, _fn(nd), nd._h, members=v, topn=10)
    rc, ids, sc, _, _ = request_call(capi, _fn(nd), nd._h, members=v, topn=10, prior_weight=float("nan"), flags=0)
    assert rc == capi.OK
    check((ids, sc), q_plain[1:3], "garbage in the padding")
    rc, ids, sc, _, _ = request_call(capi, _fn(nd), nd._h, members=v, topn=10, size=84)
    assert rc == capi.OK
    check((ids, sc), q_plain[1:3], "size 84")


def test_python_keywords_on_both_engine_classes(node):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import CosineEngine, NodeEngine
    nd, feats, lab, groups, pri = node
    names = ("query_mean_topn", "query_playlist_topn", "query_mean_topn_diverse", "query_playlist_topn_diverse",
             "query_mean_topn_capped", "query_playlist_topn_capped")
    for cls in (CosineEngine, NodeEngine):
        assert callable(getattr(cls, "set_priors"))
        for name in names:
            assert inspect.signature(getattr(cls, name)).parameters["prior_weight"].default is None, (cls, name)
    p = pri["skewed"]
    nd.set_priors(p)
    rows, wanted = [5, 777, 3000], {2, 7}
    s = scores_of(feats, feats[rows])
    check(nd.query_playlist_topn(rows, 20, prior_weight=0.25), expected_prior(s, p, 0.25, feats, lab, None, rows, 20), "by row")
    check(nd.query_mean_topn(feats[rows], 20, [1], where=WHERE, labels=wanted, prior_weight=-0.5),
          expected_prior(s, p, -0.5, feats, lab, wanted, [1], 20, WHERE), "by value")
    pl = expected_prior(s, p, 1.0, feats, lab, None, rows, 40)
    check3(nd.query_playlist_topn_diverse(rows, 10, 0.3, 40, return_mmr=True, prior_weight=1.0), expected_diverse(pl, feats, 0.3, 10), "diverse")
    got = nd.query_mean_topn_capped(feats[rows], 10, 1, 0.3, 40, exclude=rows, return_mmr=True, return_pool_rows=True, prior_weight=1.0)
    check3(got[:3], expected_diverse(pl, feats, 0.3, 10, groups, 1), "capped")
    assert got[3] == 40
    # None takes the entry point used today
    check(nd.query_playlist_topn(rows, 20, prior_weight=None), expected_prior(s, p, None, feats, lab, None, rows, 20), "None")
    with pytest.raises(capi.Mi355Error, match="prior_weight"):
        nd.query_playlist_topn(rows, 20, prior_weight=5)
    with pytest.raises(ValueError):
        nd.query_playlist_topn(rows, 20, prior_weight="1")
    nd.set_priors(None)
    with pytest.raises(capi.Mi355Error, match="has no priors"):
        nd.query_playlist_topn(rows, 20, prior_weight=1.0)


# ---- the drop-in CLI ------------------------------------------------------------------------------------------------
def _run(args, cwd):
    from spotify_recommender_amd import build
    import subprocess
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _recommended(stdout):
    out = stdout.split("Recommendations:", 1)[1]
    return [l.split("ID:", 1)[1].strip() for l in out.splitlines() if l.strip().startswith("ID:")]


def test_cli_priors(engine_lib, golden_dir, tmp_path):
    import shutil

    from spotify_recommender_amd import build
    build.build_shim()
    shutil.copy(golden_dir / "sample_songs.csv", tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    seed = "5SuOikwiRyPMVoIQDJUgSV"
    p = _run(["--playlist", seed, "-n", "1000"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    plain = _recommended(p.stdout)
    n = len(plain) + 1                                       # every song but the playlist's own
    assert n == 4
    # zero priors, and beta 0 with any priors: the plain order
    (tmp_path / "zero.txt").write_text("0\n" * n)
    (tmp_path / "ramp.txt").write_text("".join(f"{i / n:.6f}\n" for i in range(n)))
    for args in (["--priors", "zero.txt", "--prior-weight", "1"], ["--priors", "ramp.txt", "--prior-weight", "0"]):
        p = _run(["--playlist", seed, "-n", "3", *args], tmp_path)
        assert p.returncode == 0 and _recommended(p.stdout) == plain, p.stdout + p.stderr
    # a weight that swamps the similarity (steps of 4 * 0.25 between songs, cosines of non-negative rows lie in [0, 1]): the
    # songs in descending catalogue order, the playlist's own song (the first) left out; a negative weight reverses it
    p = _run(["--playlist", seed, "-n", "3", "--priors", "ramp.txt", "--prior-weight", "4"], tmp_path)
    assert p.returncode == 0 and "Prior weight: 4" in p.stdout, p.stdout + p.stderr
    top = _recommended(p.stdout)
    p = _run(["--playlist", seed, "-n", "3", "--priors", "ramp.txt", "--prior-weight", "-4"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert len(top) == 3 and sorted(top) == sorted(plain) and top == _recommended(p.stdout)[::-1] and seed not in top
    assert top[0] == "dupA"
    # with the other options of the family
    p = _run(["--playlist", seed, "-n", "3", "--priors", "ramp.txt", "--prior-weight", "0.25", "--where", "energy=0:1", "--max-per-artist", "1",
              "--genre", "rock", "--genre", "dance"], tmp_path)
    assert p.returncode == 0 and _recommended(p.stdout), p.stdout + p.stderr
    # refusals exit 1
    for args, msg in ((["--priors", "ramp.txt"], "go together"), (["--prior-weight", "1"], "go together"),
                      (["--priors", "ramp.txt", "--prior-weight", "5"], "BETA must be a number in [-4, 4]"),
                      (["--priors", "missing.txt", "--prior-weight", "1"], "cannot open the priors file")):
        p = _run(["--playlist", seed, *args], tmp_path)
        assert p.returncode == 1 and msg in p.stderr, (args, p.stderr)
    (tmp_path / "short.txt").write_text("0.5\n")
    p = _run(["--playlist", seed, "--priors", "short.txt", "--prior-weight", "1"], tmp_path)
    assert p.returncode == 1 and "holds 1 priors for" in p.stderr, p.stderr
    (tmp_path / "big.txt").write_text("1.5\n" * n)
    p = _run(["--playlist", seed, "--priors", "big.txt", "--prior-weight", "1"], tmp_path)
    assert p.returncode == 1 and "|p| <= 1" in p.stderr, p.stderr
    assert "--priors FILE --prior-weight BETA" in _run([], tmp_path).stdout
