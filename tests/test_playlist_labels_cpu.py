"""PLAYLIST REQUESTS on a host without a GPU: the playlist family within a label set through the node handle (served by the
product's CPU backend, csrc/cpu_backend.cpp), the request call against the twenty-entry-point ladder, the C-ABI's argument
errors and struct versioning, the Python keyword and the CLI's --playlist ... --genre.  Expected results are composed from
the existing checkers (tests/playlist_labels_oracle.py): equal ids, bit-equal scores, equal counts."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests.diverse_oracle import check3
from tests.labels_oracle import check
from tests.playlist_labels_oracle import (expected_diverse, expected_scored, inadmissible, request_call, scores_of, uniform_labels)


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
N_LABELS = 12


@pytest.fixture(scope="module")
def node(engine_lib, golden_dir):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = np.ascontiguousarray(np.load(golden_dir / "catalogue4096.npz")["feats"])
    lab = uniform_labels(feats.shape[0], N_LABELS, 3, unlabelled=0.05)
    groups = (np.arange(feats.shape[0]) % 7).astype(np.int32)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(lab)
        nd.set_groups(groups)
        yield nd, feats, lab, groups


def _fn(nd):
    return nd._lib.mi355rec_sharded_query_playlist_request


def test_every_field_alone_and_all_together(node):
    from spotify_recommender_amd import capi
    nd, feats, lab, groups = node
    rng = np.random.default_rng(1)
    rows = [int(r) for r in rng.choice(feats.shape[0], size=5, replace=False)]
    vecs = rng.random((4, 12), dtype=np.float32)
    w4, w5 = [1.0, -0.5, 2.0, 0.25], [1.0, 1.0, -0.5, 3.0, 1.0]
    wanted = [1, 4, 4, 9]
    s_v, s_vw, s_r, s_rw = scores_of(feats, vecs), scores_of(feats, vecs, w4), scores_of(feats, feats[rows]), scores_of(feats, feats[rows], w5)
    top = expected_scored(s_v, feats, lab, wanted, [], 40)[0]
    excl = top[::2].tolist() + [0, 1, 2]

    def call(**kw):
        rc, ids, sc, mmr, p = request_call(capi, _fn(nd), nd._h, **kw)
        assert rc == capi.OK, nd._lib.mi355rec_sharded_last_error(nd._h)
        return ids, sc, mmr, p

    for topn in (1, 10, 1024):
        # each field alone
        check(call(members=vecs, topn=topn)[:2], expected_scored(s_v, feats, lab, None, [], topn), "members")
        check(call(rows=rows, topn=topn)[:2], expected_scored(s_r, feats, lab, None, rows, topn), "rows")
        check(call(members=vecs, weights=w4, topn=topn)[:2], expected_scored(s_vw, feats, lab, None, [], topn), "weights")
        check(call(members=vecs, exclude=excl, topn=topn)[:2], expected_scored(s_v, feats, lab, None, excl, topn), "exclude")
        check(call(members=vecs, where=WHERE, topn=topn)[:2], expected_scored(s_v, feats, lab, None, [], topn, WHERE), "filter")
        check(call(members=vecs, labels=wanted, topn=topn)[:2], expected_scored(s_v, feats, lab, wanted, [], topn), "labels")
        got = call(rows=rows, labels=wanted, topn=topn)
        check(got[:2], expected_scored(s_r, feats, lab, wanted, rows, topn), "labels by row")
        assert not np.any(lab[got[0]] < 0)
        # all together
        check(call(rows=rows, weights=w5, exclude=excl, where=WHERE, labels=wanted, topn=topn)[:2],
              expected_scored(s_rw, feats, lab, wanted, rows + excl, topn, WHERE), "all together")
    for pool in (40, 1024):
        pl = expected_scored(s_rw, feats, lab, wanted, rows + excl, pool, WHERE)
        kw = dict(rows=rows, weights=w5, exclude=excl, where=WHERE, labels=wanted, topn=10, pool=pool)
        for lam in (0.0, 0.5, 1.0):
            check3(call(lam=lam, **kw)[:3], expected_diverse(pl, feats, lam, 10), f"diverse pool {pool} lambda {lam}")
            got = call(lam=lam, max_per_group=1, **kw)
            check3(got[:3], expected_diverse(pl, feats, lam, 10, groups, 1), f"capped pool {pool} lambda {lam}")
            assert got[3] == pl[0].size
    # counts: fewer admissible rows than topn, a label without rows, every label on the labelled rows
    few = int(np.count_nonzero(lab == 4))
    assert 0 < few < 1024
    ids = call(members=vecs, labels=[4], topn=1024)[0]
    assert ids.size == few and set(ids.tolist()) == set(np.flatnonzero(lab == 4).tolist())
    assert call(members=vecs, labels=[500, 501], topn=10)[0].size == 0
    ids = call(members=vecs, labels=range(N_LABELS), topn=1024)[0]
    assert not set(ids.tolist()) & set(inadmissible(feats, lab, range(N_LABELS)).tolist())
    # K = 1 by row with a label set: the label route's query
    for q in (0, 99, 4095):
        check(call(rows=[q], labels=wanted, topn=50)[:2], nd.query_row_topn_labels(q, wanted, 50), f"row {q}")


LADDER = [(by, level) for by in ("mean", "playlist") for level in ("", "_where", "_weighted", "_diverse", "_capped")]


@pytest.mark.parametrize("by,level", LADDER)
def test_old_entry_points_are_special_cases_of_the_request(node, by, level):
    """The node handle's ten entry points (the CPU backend's: the single handle's ten need a device, tests/test_gpu_playlist_labels.py)."""
    from spotify_recommender_amd import capi
    nd, feats, lab, groups = node
    rng = np.random.default_rng(len(level))
    rows = [int(r) for r in rng.choice(feats.shape[0], size=6, replace=False)]
    m = dict(rows=rows) if by == "playlist" else dict(members=feats[rows])
    members = rows if by == "playlist" else feats[rows]
    w = rng.normal(0.0, 1.0, 6).astype(np.float32)
    excl = [int(e) for e in rng.integers(0, feats.shape[0], size=50)]
    rank = ("", "_where", "_weighted", "_diverse", "_capped").index(level)
    kw, old = dict(exclude=excl), dict(exclude=excl)
    if rank >= 1:
        kw["where"] = old["where"] = WHERE
    if rank >= 2:
        kw["weights"] = old["weights"] = w
    if rank >= 3:
        kw.update(lam=0.4, pool=64)
        old.update(lam=0.4, pool=64, return_mmr=True)
    if rank == 4:
        kw["max_per_group"] = old["max_per_group"] = 2
        old["return_pool_rows"] = True
    for topn in (1, 10, 64):
        want = getattr(nd, f"query_{by}_topn{level if rank >= 3 else ''}")(members, topn, **old)
        rc, ids, sc, mmr, p = request_call(capi, _fn(nd), nd._h, topn=topn, **m, **kw)
        assert rc == capi.OK
        check((ids, sc), want[:2], f"{by}{level} top-{topn}")
        if rank >= 3:
            check3((ids, sc, mmr), want[:3], f"{by}{level} top-{topn}")
        if rank == 4:
            assert p == want[3]


def test_argument_errors(node):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd, feats, lab, groups = node

    def refused(msg, h=None, **kw):
        h = h or nd
        rc = request_call(capi, _fn(h), h._h, **kw)[0]
        text = h._lib.mi355rec_sharded_last_error(h._h).decode()
        assert rc == capi.ERR_INVALID_ARG and msg in text, (kw.keys(), rc, text)

    v = feats[:2]
    refused("n_labels must be positive, got -1", members=v, n_labels=-1)
    refused("null label set", members=v, n_labels=3)
    refused("n_labels must be positive, got 0", members=v, labels=[])
    refused("label 1024 out of [0, 1024)", members=v, labels=[1, 1024])
    refused("label -1 out of [0, 1024)", members=v, labels=[-1])
    with NodeEngine(feats[:100], placement=capi.PLACEMENT_AUTO) as fresh:
        refused("has no labels", h=fresh, members=v, labels=[1])
        refused("has no labels", h=fresh, rows=[1, 2], labels=[1], lam=0.5, pool=20)
        assert request_call(capi, _fn(fresh), fresh._h, members=v)[0] == capi.OK      # without a set, no labels are needed
    # everything the family already refuses
    refused("playlist of 0 songs", members=v, k=0)
    refused("playlist of 33 songs", rows=list(range(33)))
    refused("topn 0 out of", members=v, topn=0)
    refused("topn 1025 out of", members=v, topn=1025)
    refused("n_exclude -1 out of", members=v, n_exclude=-1)
    refused("null exclusion list", members=v, n_exclude=2)
    refused("excluded row", members=v, exclude=[-5])
    refused("Invalid song index: 4096", rows=[1, 4096])
    refused("lambda", members=v, lam=1.5, pool=20)
    refused("pool 5 out of", members=v, lam=0.5, pool=5)
    refused("max_per_group must be positive", members=v, lam=0.5, pool=20, max_per_group=0)
    refused("weight", members=v, weights=[np.nan, 1.0])
    flt = capi.Filter()
    flt.active = 1 << 12
    refused("", members=v, where=flt)
    refused("null argument", topn=10)                                                  # neither members nor rows
    refused("by value and by row", members=v, rows=[1, 2])
    refused("unknown flags", members=v, flags=8)
    refused("MI355REC_PQ_CAPPED needs", members=v, flags=capi.PQ_CAPPED)
    L = nd._lib
    q = capi.PlaylistQuery()
    q.size = ctypes.sizeof(q)
    assert L.mi355rec_sharded_query_playlist_request(nd._h, ctypes.byref(q), None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_sharded_query_playlist_request(nd._h, None, None) == capi.ERR_INVALID_ARG
    res = capi.PlaylistResult()                                                         # a null out_idx
    v2 = np.ascontiguousarray(v)
    q.members, q.k, q.topn = v2.ctypes.data_as(ctypes.c_void_p), 2, 5
    assert L.mi355rec_sharded_query_playlist_request(nd._h, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG


def test_struct_versioning(node):
    from spotify_recommender_amd import capi
    nd, feats, lab, groups = node
    full = ctypes.sizeof(capi.PlaylistQuery)
    v, wanted = feats[:3], [1, 2]
    s = scores_of(feats, v)
    kw = dict(members=v, labels=wanted, topn=10, lam=0.5, pool=40, max_per_group=1)
    # the whole struct
    rc, ids, sc, mmr, p = request_call(capi, _fn(nd), nd._h, **kw)
    assert rc == capi.OK
    check3((ids, sc, mmr), expected_diverse(expected_scored(s, feats, lab, wanted, [], 40), feats, 0.5, 10, groups, 1), "full")
    # an older caller whose struct ended before max_per_group: the field reads as zero (and a capped call is then refused) ...
    cut = capi.PlaylistQuery.max_per_group.offset
    assert request_call(capi, _fn(nd), nd._h, size=cut, **kw)[0] == capi.ERR_INVALID_ARG
    assert "max_per_group must be positive, got 0" in nd._lib.mi355rec_sharded_last_error(nd._h).decode()
    # ... before the label set's count and topn: both read as zero
    assert request_call(capi, _fn(nd), nd._h, size=capi.PlaylistQuery.n_labels.offset, members=v, labels=wanted, topn=10)[0] == capi.ERR_INVALID_ARG
    # ... before lambda: a plain call with every field in front of it intact
    rc, ids, sc, _, _ = request_call(capi, _fn(nd), nd._h, size=capi.PlaylistQuery.lambda_.offset, members=v, labels=wanted, topn=10)
    assert rc == capi.OK
    check((ids, sc), expected_scored(s, feats, lab, wanted, [], 10), "cut before lambda")
    # sizes the library cannot read
    for size in (0, 3, 12, 20, cut + 2, full + 1, full + 64):   # (12, 20, cut + 2: inside a field)
        assert request_call(capi, _fn(nd), nd._h, size=size, **kw)[0] == capi.ERR_INVALID_ARG
        assert "playlist query of size" in nd._lib.mi355rec_sharded_last_error(nd._h).decode()


def test_python_keyword_on_both_engine_classes(node):
    import inspect

    from spotify_recommender_amd.engine import CosineEngine, NodeEngine
    nd, feats, lab, groups = node
    names = ("query_mean_topn", "query_playlist_topn", "query_mean_topn_diverse", "query_playlist_topn_diverse",
             "query_mean_topn_capped", "query_playlist_topn_capped")
    for cls in (CosineEngine, NodeEngine):
        for name in names:
            assert inspect.signature(getattr(cls, name)).parameters["labels"].default is None, (cls, name)
    rows, wanted = [5, 777, 3000], {2, 7}
    s = scores_of(feats, feats[rows])
    check(nd.query_playlist_topn(rows, 20, labels=wanted), expected_scored(s, feats, lab, wanted, rows, 20), "by row")
    check(nd.query_mean_topn(feats[rows], 20, [1], where=WHERE, labels=wanted), expected_scored(s, feats, lab, wanted, [1], 20, WHERE), "by value")
    pl = expected_scored(s, feats, lab, wanted, rows, 40)
    check3(nd.query_playlist_topn_diverse(rows, 10, 0.3, 40, return_mmr=True, labels=wanted), expected_diverse(pl, feats, 0.3, 10), "diverse")
    got = nd.query_mean_topn_capped(feats[rows], 10, 1, 0.3, 40, exclude=rows, return_mmr=True, return_pool_rows=True, labels=wanted)
    check3(got[:3], expected_diverse(pl, feats, 0.3, 10, groups, 1), "capped")
    assert got[3] == 40
    # None takes the old entry point; an empty set is refused by the library
    check(nd.query_playlist_topn(rows, 20, labels=None), expected_scored(s, feats, lab, None, rows, 20), "None")
    from spotify_recommender_amd import capi
    with pytest.raises(capi.Mi355Error, match="n_labels must be positive"):
        nd.query_playlist_topn(rows, 20, labels=[])


# ---- the drop-in CLI ------------------------------------------------------------------------------------------------
def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _recommended(stdout):
    out = stdout.split("Recommendations:", 1)[1]
    ids = [l.split("ID:", 1)[1].strip() for l in out.splitlines() if l.strip().startswith("ID:")]
    genres = [l.split("Genre:", 1)[1].strip() for l in out.splitlines() if "Genre:" in l]
    return ids, genres


def test_cli_playlist_within_genres(engine_lib, golden_dir, tmp_path):
    import shutil

    from spotify_recommender_amd import build
    build.build_shim()
    shutil.copy(golden_dir / "sample_songs.csv", tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    seed = "5SuOikwiRyPMVoIQDJUgSV"
    # what the CLI serves: every other song in similarity order (the restricted answers are this list, filtered)
    p = _run(["--playlist", seed, "-n", "10"], tmp_path)
    assert p.returncode == 0 and "Restricted to genres" not in p.stdout, p.stdout + p.stderr
    everything = list(zip(*_recommended(p.stdout)))
    by_genre = {}
    for tid, genre in everything:
        by_genre.setdefault(genre, []).append(tid)
    assert len(by_genre["dance"]) == 2 and len(by_genre["rock"]) >= 1, by_genre
    # a dance song, recommendations from rock only: the playlist's own song need not be in the genre
    p = _run(["--playlist", seed, "--genre", "Rock", "-n", "5"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    ids, genres = _recommended(p.stdout)
    assert "Restricted to genres: Rock" in p.stdout
    assert ids == by_genre["rock"] and set(genres) == {"rock"}
    # its own genre: the member is never returned
    p = _run(["--playlist", seed, "--genre", "dance", "-n", "5"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    ids, genres = _recommended(p.stdout)
    assert ids == by_genre["dance"] and seed not in ids and set(genres) == {"dance"}
    # two genres, with the combinations the --song mode refuses
    plain = _recommended(_run(["--playlist", seed, "--genre", "rock", "--genre", "dance", "-n", "3"], tmp_path).stdout)[0]
    assert plain == [tid for tid, genre in everything if genre in ("rock", "dance")][:3] and len(plain) == 3
    p = _run(["--playlist", seed, "--genre", "rock", "--genre", "dance", "-n", "3", "--diverse", "1.0"], tmp_path)
    assert p.returncode == 0 and _recommended(p.stdout)[0] == plain            # lambda 1 is the plain result
    p = _run(["--playlist", seed, "--genre", "rock", "--genre", "dance", "-n", "4", "--where", "energy=0:1", "--max-per-artist", "1",
              "--dislike", by_genre["rock"][0]], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    ids, genres = _recommended(p.stdout)
    assert ids and set(genres) <= {"rock", "dance"} and by_genre["rock"][0] not in ids and seed not in ids
    # an unknown genre exits 1
    p = _run(["--playlist", seed, "--genre", "polka"], tmp_path)
    assert p.returncode == 1 and "Unknown genre 'polka'" in p.stderr
    # without --genre nothing changes
    p = _run(["--playlist", seed, "-n", "3"], tmp_path)
    assert p.returncode == 0 and "Restricted to genres" not in p.stdout
    # the --song / --id modes keep their refusals, and the usage says what to use instead
    for extra, msg in ((["--where", "energy=0:1"], "--where cannot be combined with --genre"),
                       (["--diverse", "0.5"], "--diverse cannot be combined with --genre"),
                       (["--max-per-artist", "1"], "--max-per-artist cannot be combined with --genre")):
        p = _run(["--id", seed, "--genre", "rock", *extra], tmp_path)
        assert p.returncode == 1 and msg in p.stderr, p.stderr
    assert "--playlist <one id> --genre" in _run([], tmp_path).stdout
