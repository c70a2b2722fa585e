"""WEIGHTED PLAYLISTS on a host without a GPU: signed per-song weights through the node handle (served by the product's CPU
backend, csrc/cpu_backend.cpp), the C-ABI's argument errors, the C++ drop-in through its shim and the CLI's --dislike /
--weights.  Checked against the oracle (tests/weighted_oracle.py): identical ids, bit-equal scores."""
import ctypes
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import catalogue, check
from tests.playlist_oracle import expected_rows as unweighted_rows
from tests.weighted_oracle import expected, expected_rows, weight_kinds, weighted_scores


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}


@pytest.fixture(scope="module")
def node(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, _ = catalogue(20_000, 114, seed=13)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        yield nd, feats


@pytest.mark.parametrize("k", [1, 2, 7, 32])
@pytest.mark.parametrize("topn", [1, 10, 1024])
def test_weighted_playlists_match_the_oracle(node, k, topn):
    nd, feats = node
    rng = np.random.default_rng(k * 1000 + topn)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    vecs = rng.random((k, 12), dtype=np.float32)
    excl = rng.integers(0, feats.shape[0], size=300)
    for kind, w in weight_kinds(rng, k):
        what = f"k={k} top-{topn} {kind}"
        check(nd.query_playlist_topn(rows, topn, weights=w), expected_rows(feats, rows, w, [], topn), what + " by row")
        check(nd.query_mean_topn(vecs, topn, weights=w), expected(feats, vecs, w, [], topn), what + " by value")
        check(nd.query_mean_topn(vecs, topn, excl, weights=w), expected(feats, vecs, w, excl, topn), what + " excluded")
        check(nd.query_playlist_topn(rows, topn, excl, where=WHERE, weights=w), expected_rows(feats, rows, w, excl, topn, WHERE),
              what + " excluded, filtered")
        check(nd.query_mean_topn(vecs, topn, where=WHERE, weights=w), expected(feats, vecs, w, [], topn, WHERE),
              what + " by value, filtered")


@pytest.mark.parametrize("k", [1, 2, 7, 32])
def test_identities_all_ones_and_powers_of_two(node, k):
    nd, feats = node
    rng = np.random.default_rng(70 + k)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    excl = rng.integers(0, feats.shape[0], size=50)
    ones = np.ones(k, np.float32)
    for topn in (1, 10, 1024):
        want = nd.query_playlist_topn(rows, topn, excl)
        check(want, unweighted_rows(feats, rows, excl.tolist(), topn), "the unweighted call")
        check(nd.query_playlist_topn(rows, topn, excl, weights=ones), want, f"k={k} top-{topn} weights of 1")
        check(nd.query_mean_topn(feats[rows], topn, excl, weights=ones), nd.query_mean_topn(feats[rows], topn, excl), "by value")
        check(nd.query_playlist_topn(rows, topn, excl, where=WHERE, weights=ones), nd.query_playlist_topn(rows, topn, excl, where=WHERE),
              "filtered")
        for kind, w in weight_kinds(rng, k):
            base = nd.query_playlist_topn(rows, topn, excl, weights=w)
            for p in (8, -8):
                check(nd.query_playlist_topn(rows, topn, excl, weights=w * np.float32(2.0 ** p)), base, f"{kind} x 2^{p}")


def _raw(L, fn, h, members, weights, k, topn, filt=None):
    idx = np.empty(max(topn, 1), np.int64)
    sc = np.empty(max(topn, 1), np.float32)
    c = ctypes.c_int(0)
    rc = getattr(L, fn)(h, members.ctypes.data_as(ctypes.c_void_p), None if weights is None else weights.ctypes.data_as(ctypes.c_void_p),
                        k, None, 0, filt, topn, idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c))
    return rc, idx[:c.value].copy(), sc[:c.value].copy()


def test_null_weights_are_the_where_call(node, engine_lib):
    from spotify_recommender_amd.engine import make_filter
    nd, feats = node
    rows = np.array([5, 777, 12_345], np.int64)
    flt = make_filter(WHERE)
    for filt, where in ((None, None), (ctypes.byref(flt), WHERE)):
        rc, idx, sc = _raw(engine_lib, "mi355rec_sharded_query_playlist_topn_weighted", nd._h, rows, None, 3, 40, filt)
        assert rc == 0
        check((idx, sc), nd.query_playlist_topn(rows, 40, where=where), "NULL weights by row")
        vecs = np.ascontiguousarray(feats[rows])
        rc, idx, sc = _raw(engine_lib, "mi355rec_sharded_query_mean_topn_weighted", nd._h, vecs, None, 3, 40, filt)
        assert rc == 0
        check((idx, sc), nd.query_mean_topn(vecs, 40, where=where), "NULL weights by value")


def test_a_single_dislike_reverses_the_ranking(node):
    nd, feats = node
    for q in (0, 99, 12_345):
        c = oracle.scores(feats, feats[q])
        idx, sc = nd.query_playlist_topn([q], 200, weights=[-1.0])
        check((idx, sc), expected_rows(feats, [q], [-1.0], [], 200), f"row {q}")
        assert np.array_equal(sc, -c[idx] + np.float32(0))                      # score = -c exactly
        assert np.all(np.diff(sc) <= 0)
        ties = np.flatnonzero(np.diff(sc) == 0)
        assert np.all(idx[ties] < idx[ties + 1])                                # ties by row ascending
    # the zero rows (10..13) score -0.0 against everything: reported as +0.0
    idx, sc = nd.query_mean_topn(np.zeros((1, 12), np.float32), 30, weights=[-1.0])
    assert idx.tolist() == list(range(30)) and not sc.view(np.uint32).any()


def test_a_pair_that_cancels_scores_zero_everywhere(node):
    nd, feats = node
    a = 4242
    idx, sc = nd.query_playlist_topn([a, a], 50, weights=[1.0, -1.0])
    assert idx.tolist() == [i for i in range(51) if i != a][:50]
    assert not sc.view(np.uint32).any()                                         # +0.0 each
    idx, sc = nd.query_mean_topn(feats[[a, a]], 1024, weights=[-3.0, 3.0])
    assert idx.tolist() == list(range(1024)) and not sc.view(np.uint32).any()


def test_zero_weight_and_zero_row_members(node):
    nd, feats = node
    a, b, z = 5, 777, 3000
    got = nd.query_playlist_topn([a, z, b], 60, weights=[1.0, 0.0, 0.5])
    check(got, expected_rows(feats, [a, z, b], [1.0, 0.0, 0.5], [], 60), "a zero-weight member")
    assert z not in got[0].tolist()                                             # still excluded
    # ... and it changes nothing beyond W: the same ranking as without it, with z taken out
    without = nd.query_playlist_topn([a, b], 61, weights=[1.0, 0.5])[0].tolist()
    assert got[0].tolist() == [i for i in without if i != z][:60]
    # a disliked member is excluded too
    got = nd.query_playlist_topn([a, b], 1024, weights=[1.0, -1.0])
    assert b not in got[0].tolist() and a not in got[0].tolist()
    # zero rows (10..13 of the catalogue) as members: they score 0 and only their weight counts, in W
    for w in ([1.0, 2.0], [-1.0, 2.0], [1.0, -0.25]):
        check(nd.query_playlist_topn([10, a], 40, weights=w), expected_rows(feats, [10, a], w, [], 40), f"a zero row, {w}")
    check(nd.query_playlist_topn([10, 11], 40, weights=[1.0, -1.0]), expected_rows(feats, [10, 11], [1.0, -1.0], [], 40), "zero rows only")


def test_ties_and_duplicate_rows_keep_the_canonical_order(node):
    nd, feats = node
    # rows 100..109 are copies of 99: liked and disliked copies cancel exactly, the third member decides
    w = [1.0, -1.0, 0.75]
    check(nd.query_playlist_topn([99, 100, 555], 64, weights=w), expected_rows(feats, [99, 100, 555], w, [], 64), "copies")
    idx, sc = nd.query_playlist_topn([99], 20, weights=[0.125])
    assert idx[:10].tolist() == list(range(100, 110)), idx                      # the copies: score 1.0 each, rows ascending


def test_clustered_catalogue_likes_in_one_cluster_dislikes_in_another(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    from spotify_recommender_amd.synth import clustered_catalogue
    n, clusters = 60_000, 30
    feats = clustered_catalogue(n, 0.03, seed=4242 + clusters, clusters=clusters, contiguous=True, ramp=False, device="cpu").numpy()
    per = n // clusters
    rng = np.random.default_rng(30)
    liked = 17 * per + rng.choice(per // 2, size=7, replace=False) + per // 4
    disliked = 5 * per + rng.choice(per // 2, size=3, replace=False) + per // 4
    rows = np.concatenate([liked, disliked])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        for dw in (0.5, 1.0):
            w = np.array([1.0] * 7 + [-dw] * 3, np.float32)
            for topn in (10, 1024):
                check(nd.query_playlist_topn(rows, topn, weights=w), expected_rows(feats, rows, w, [], topn), f"-{dw} top-{topn}")
            check(nd.query_playlist_topn(rows, 100, [int(liked[0]) + 1], where={"tempo": (0.05, 0.95)}, weights=w),
                  expected_rows(feats, rows, w, [int(liked[0]) + 1], 100, {"tempo": (0.05, 0.95)}), "filtered")


def test_argument_errors(node, engine_lib):
    from spotify_recommender_amd import capi
    nd, feats = node
    n = feats.shape[0]
    ones2 = np.ones((2, 12), np.float32)
    bad_calls = [
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[1.0, np.nan]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[np.inf, 1.0]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[1.0, -np.inf]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[1.0, 1.5e6]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[-1.000001e6, 1.0]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[0.0, 0.0]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[-0.0, 0.0]),
        lambda: nd.query_playlist_topn([1, 2], 10, weights=[4e-7, -4e-7]),
        lambda: nd.query_mean_topn(ones2, 10, weights=[np.nan, 1.0]),
        lambda: nd.query_mean_topn(ones2, 10, weights=[0.0, 0.0]),
        lambda: nd.query_mean_topn(ones2, 10, weights=[2e6, 0.0]),
        # the playlist and filter cases still hold on the weighted entry points
        lambda: nd.query_playlist_topn(list(range(33)), 10, weights=[1.0] * 33),
        lambda: nd.query_playlist_topn([1], 0, weights=[1.0]),
        lambda: nd.query_playlist_topn([1], 1025, weights=[1.0]),
        lambda: nd.query_playlist_topn([n], 10, weights=[1.0]),
        lambda: nd.query_playlist_topn([1], 10, [n], weights=[1.0]),
        lambda: nd.query_playlist_topn([1], 10, list(range(1025)), weights=[1.0]),
        lambda: nd.query_playlist_topn([1], 10, where={1: (0.9, 0.1)}, weights=[1.0]),
        lambda: nd.query_mean_topn(ones2, 10, where={1: (np.nan, 1.0)}, weights=[1.0, 1.0]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(capi.Mi355Error) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARG, i
        assert str(e.value), i
    # a weight list of the wrong length never reaches the library
    for bad in ([1.0], [1.0, 1.0, 1.0], []):
        with pytest.raises(ValueError):
            nd.query_playlist_topn([1, 2], 10, weights=bad)
    # raw calls: a message in last_error
    L = engine_lib
    rows = np.array([1, 2], np.int64)
    for w in ([np.nan, 1.0], [0.0, 0.0], [1e7, 1.0]):
        for fn, members in (("mi355rec_sharded_query_playlist_topn_weighted", rows),
                            ("mi355rec_sharded_query_mean_topn_weighted", ones2)):
            rc, _, _ = _raw(L, fn, nd._h, members, np.array(w, np.float32), 2, 10)
            assert rc == capi.ERR_INVALID_ARG
            assert b"weight" in L.mi355rec_sharded_last_error(nd._h)
    # the edges are allowed: |w| = 1e6 and W = 1e-6
    for w in ([1e6, -1e6], [1e-6, 0.0], [5e-7, -5e-7]):
        check(nd.query_playlist_topn([1, 2], 10, weights=w), expected_rows(feats, [1, 2], w, [], 10), f"edge {w}")
    # a good call after the errors still answers
    check(nd.query_playlist_topn([1, 2], 10, weights=[1.0, -0.5]), expected_rows(feats, [1, 2], [1.0, -0.5], [], 10), "after errors")


# ---- the C++ drop-in (through its shim) and the CLI ---------------------------------------------------------------------
def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _shim():
    from spotify_recommender_amd import build
    build.build_shim()
    shim = ctypes.CDLL(str(build.LIB_SHIM))
    P, I = ctypes.c_void_p, ctypes.c_int
    shim.shim_load.restype = P
    shim.shim_load.argtypes = [ctypes.c_char_p]
    shim.shim_free.argtypes = [P]
    shim.shim_initialize.argtypes = [P]
    shim.shim_song_count.restype = ctypes.c_int64
    shim.shim_song_count.argtypes = [P]
    shim.shim_song_features.argtypes = [P, ctypes.c_int64, P, ctypes.POINTER(I)]
    shim.shim_recommend_for_playlist_weighted.restype = ctypes.c_int64
    shim.shim_recommend_for_playlist_weighted.argtypes = [P, P, I, P, I, I, P, P, P, I, P, I, P, P, ctypes.c_int64]
    shim.shim_recommend_for_taste.restype = ctypes.c_int64
    shim.shim_recommend_for_taste.argtypes = [P, P, I, P, I, I, ctypes.c_float, P, P, ctypes.c_int64]
    return shim


def _served_matrix(shim, path):
    h = shim.shim_load(str(path).encode())
    assert h
    try:
        n = shim.shim_song_count(h)
        feats = np.zeros((n, 12), np.float32)
        g = ctypes.c_int(0)
        for i in range(n):
            shim.shim_song_features(h, i, feats[i].ctypes.data, ctypes.byref(g))
    finally:
        shim.shim_free(h)
    return feats


def _ids(stdout):
    return [l.split("ID:", 1)[1].strip() for l in stdout.split("Recommendations:", 1)[1].splitlines() if l.strip().startswith("ID:")]


@pytest.fixture()
def sample(engine_lib, tmp_path):
    from tests.test_playlist_cpu import _write_csv
    shim = _shim()
    _write_csv(tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    feats = _served_matrix(shim, tmp_path / "songs_data.bin")
    track_ids = [l.split(",", 1)[0] for l in (tmp_path / "songs.csv").read_text().splitlines()[1:]]
    return shim, feats, track_ids, tmp_path


def test_cli_dislike_and_weights(sample):
    shim, feats, t, cwd = sample
    liked, disliked = [0, 3, 6], [9, 12]
    lk, dl = ",".join(t[i] for i in liked), ",".join(t[i] for i in disliked)
    # --dislike at the default weight 0.5
    p = _run(["--playlist", lk, "--dislike", dl, "-n", "5"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    want = expected_rows(feats, liked + disliked, [1, 1, 1, -0.5, -0.5], [], 5)[0]
    assert _ids(p.stdout) == [t[i] for i in want], p.stdout
    assert "weight -0.5" in p.stdout
    # --dislike-weight, --weights and --where together
    p = _run(["--playlist", lk, "--dislike", dl, "--dislike-weight", "1", "--weights", "1,1,0.25", "--where", "energy=0:0.9", "-n", "4"],
             cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    want = expected_rows(feats, liked + disliked, [1, 1, 0.25, -1, -1], [], 4, {"energy": (0.0, 0.9)})[0]
    assert want.size > 0 and _ids(p.stdout) == [t[i] for i in want], p.stdout
    # --weights alone
    p = _run(["--playlist", lk, "--weights", "2,0.5,1", "-n", "5"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in expected_rows(feats, liked, [2, 0.5, 1], [], 5)[0]], p.stdout
    # the plain playlist is unchanged by the new options' absence
    p = _run(["--playlist", lk, "-n", "5"], cwd)
    assert _ids(p.stdout) == [t[i] for i in unweighted_rows(feats, liked, [], 5)[0]], p.stdout
    # refusals: exit status 1 and a message
    for bad, msg in ((["--weights", "1,1"], "weights"),                       # the wrong length
                     (["--weights", "1,1,1,1"], "weights"),
                     (["--weights", "1,x,1"], "not a number"),
                     (["--dislike", f"{t[9]},nosuchid"], "nosuchid"),           # an unknown id
                     (["--dislike"], "needs a value"),
                     (["--dislike", dl, "--dislike-weight", "-1"], "--dislike-weight"),
                     (["--weights", "0,0,0"], "weights")):                    # all zero: refused by the library
        p = _run(["--playlist", lk, *bad], cwd)
        assert p.returncode == 1, (bad, p.stdout)
        assert msg in p.stderr, (bad, p.stderr)
    assert "--dislike" in _run([], cwd).stdout


def test_recommender_weighted_through_the_shim(sample):
    shim, feats, t, cwd = sample
    h = shim.shim_load(str(cwd / "songs_data.bin").encode())
    assert h
    try:
        assert shim.shim_initialize(h) == 1

        def weighted(songs, weights, topn, ranges=(), exclude=()):
            s, w = np.array(songs, np.int32), np.array(weights, np.float32)
            f = np.array([r[0] for r in ranges] or [0], np.int32)
            lo = np.array([r[1] for r in ranges] or [0], np.float32)
            hi = np.array([r[2] for r in ranges] or [0], np.float32)
            ex = np.array(list(exclude) or [0], np.int32)
            out, sc = np.full(32, -7, np.int32), np.zeros(32, np.float32)
            n = shim.shim_recommend_for_playlist_weighted(h, s.ctypes.data, len(songs), w.ctypes.data, len(weights), topn, f.ctypes.data,
                                                          lo.ctypes.data, hi.ctypes.data, len(ranges), ex.ctypes.data, len(exclude),
                                                          out.ctypes.data, sc.ctypes.data, 32)
            return out[:max(n, 0)].astype(np.int64), sc[:max(n, 0)]

        def taste(liked, disliked, topn, dw):
            a, b = np.array(liked or [0], np.int32), np.array(disliked or [0], np.int32)
            out, sc = np.full(32, -7, np.int32), np.zeros(32, np.float32)
            n = shim.shim_recommend_for_taste(h, a.ctypes.data, len(liked), b.ctypes.data, len(disliked), topn, dw, out.ctypes.data,
                                              sc.ctypes.data, 32)
            return out[:max(n, 0)].astype(np.int64), sc[:max(n, 0)]

        w = [1.0, -0.75, 0.25]
        check(weighted([0, 3, 5], w, 10), expected_rows(feats, [0, 3, 5], w, [], 10), "weighted")
        check(weighted([0, 3, 5], w, 10, [(1, 0.0, 0.8)], [1, 2]), expected_rows(feats, [0, 3, 5], w, [1, 2], 10, {1: (0.0, 0.8)}),
              "weighted, filtered, excluded")
        check(weighted([0, 3], [1.0, 1.0], 10), unweighted_rows(feats, [0, 3], [], 10), "weights of 1")
        check(taste([0, 3], [7], 10, 0.5), expected_rows(feats, [0, 3, 7], [1, 1, -0.5], [], 10), "taste")
        check(taste([0, 3], [], 10, 0.5), unweighted_rows(feats, [0, 3], [], 10), "taste without dislikes")
        check(taste([2], [7, 8], 10, 0.0), expected_rows(feats, [2, 7, 8], [1, 0, 0], [], 10), "taste, dislikeWeight 0")
        # bad input: {} (and a message on stderr), as the class reports every other bad input
        assert weighted([0, 3], [1.0], 10)[0].size == 0                     # the wrong length
        assert weighted([0, 3], [1.0, 1.0, 1.0], 10)[0].size == 0
        assert weighted([0, 3], [np.nan, 1.0], 10)[0].size == 0
        assert weighted([0, 3], [0.0, 0.0], 10)[0].size == 0
        assert weighted([0, 3], [1e7, 1.0], 10)[0].size == 0
        assert taste([], [7], 10, 0.5)[0].size == 0
        assert taste([0], [7], 10, -1.0)[0].size == 0
        check(weighted([0, 3, 5], w, 10), expected_rows(feats, [0, 3, 5], w, [], 10), "after the refusals")
    finally:
        shim.shim_free(h)


def test_the_oracle_formula_rounds_after_every_operation():
    """weighted_scores is multiply, round, add, round (a fused multiply-add would differ on some row)."""
    feats = oracle.mt19937_uniform(21, 4096)
    rng = np.random.default_rng(21)
    members, w = feats[rng.integers(0, 4096, 7)], rng.normal(0, 1, 7).astype(np.float32)
    got = weighted_scores(feats, members, w)
    c = np.stack([oracle.scores(feats, np.ascontiguousarray(q)) for q in members]).astype(np.float64)
    exact = (w.astype(np.float64)[:, None] * c).sum(0) / np.abs(w.astype(np.float64)).sum()
    assert np.abs(got - exact).max() < 40 * 2.0 ** -24
    assert got.dtype == np.float32 and np.all(np.abs(got) <= 1.0)
