"""WEIGHTED PLAYLISTS on the MI355X: signed per-song weights through playlist_scan_kernel (csrc/playlist.hip.h), checked bit
for bit against the oracle (tests/weighted_oracle.py) on a single handle with the 8-bit replica (1 M rows) and without it
(50 000 rows: every row exact), a lane, virtual shards {0, 0, 0} and replicated placement; the two identities (weights of 1
are the unweighted call, a power of two changes nothing); a lone dislike; members that cancel; zero weights and zero rows;
a clustered catalogue with likes in one cluster and dislikes in another; the argument errors; the counters."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import check
from tests.playlist_oracle import expected_rows as unweighted_rows
from tests.weighted_oracle import expected, expected_rows, weight_kinds

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
N_BIG, N_SMALL = 1_000_000, 50_000   # above and below the 65 536 rows from which a handle keeps an 8-bit replica


def _special_rows(feats):
    feats[10:14] = 0.0                  # zero rows
    feats[100:110] = feats[99]          # copies of row 99: ties broken by row
    return np.ascontiguousarray(feats)


@pytest.fixture(scope="module")
def big(engine_lib):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine
    feats = _special_rows(oracle.mt19937_uniform(78, N_BIG))
    with CosineEngine(feats) as eng:
        yield eng, feats


@pytest.fixture(scope="module")
def small(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    feats = _special_rows(oracle.mt19937_uniform(6, N_SMALL))
    with CosineEngine(feats) as eng:
        yield eng, feats


@pytest.fixture(params=["replica", "exact"])
def handle(request):
    return request.getfixturevalue("big" if request.param == "replica" else "small")


@pytest.mark.parametrize("k", [1, 2, 7, 32])
def test_weighted_playlists_match_the_oracle(handle, k):
    eng, feats = handle
    n = feats.shape[0]
    rng = np.random.default_rng(200 + k)
    rows = rng.choice(n, size=k, replace=False)
    vecs = rng.random((k, 12), dtype=np.float32)
    excl = rng.integers(0, n, size=1000)
    for kind, w in weight_kinds(rng, k):
        top = expected_rows(feats, rows, w, [], 600)[0]
        excl[:300] = top[::2][:300]                        # drawn from the true top
        for topn in (1, 10, 1024):
            what = f"n={n} k={k} {kind} top-{topn}"
            check(eng.query_playlist_topn(rows, topn, weights=w), expected_rows(feats, rows, w, [], topn), what + " by row")
            check(eng.query_mean_topn(vecs, topn, weights=w), expected(feats, vecs, w, [], topn), what + " by value")
            check(eng.query_playlist_topn(rows, topn, excl, weights=w), expected_rows(feats, rows, w, excl, topn), what + " excluded")
            check(eng.query_playlist_topn(rows, topn, excl, where=WHERE, weights=w), expected_rows(feats, rows, w, excl, topn, WHERE),
                  what + " excluded, filtered")
            check(eng.query_mean_topn(vecs, topn, where=WHERE, weights=w), expected(feats, vecs, w, [], topn, WHERE),
                  what + " by value, filtered")


@pytest.mark.parametrize("k", [1, 2, 7, 32])
def test_identities_all_ones_and_powers_of_two(handle, k):
    eng, feats = handle
    rng = np.random.default_rng(80 + k)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    excl = rng.integers(0, feats.shape[0], size=50)
    ones = np.ones(k, np.float32)
    for topn in (1, 10, 1024):
        want = eng.query_playlist_topn(rows, topn, excl)
        check(want, unweighted_rows(feats, rows, excl.tolist(), topn), "the unweighted call")
        check(eng.query_playlist_topn(rows, topn, excl, weights=ones), want, f"k={k} top-{topn} weights of 1")
        check(eng.query_mean_topn(feats[rows], topn, excl, weights=ones), eng.query_mean_topn(feats[rows], topn, excl), "by value")
        check(eng.query_playlist_topn(rows, topn, excl, where=WHERE, weights=ones), eng.query_playlist_topn(rows, topn, excl, where=WHERE),
              "filtered")
        for kind, w in weight_kinds(rng, k):
            base = eng.query_playlist_topn(rows, topn, excl, weights=w)
            for p in (8, -8):
                check(eng.query_playlist_topn(rows, topn, excl, weights=w * np.float32(2.0 ** p)), base, f"{kind} x 2^{p}")


def _raw(L, fn, h, members, weights, k, topn, filt=None):
    idx = np.empty(max(topn, 1), np.int64)
    sc = np.empty(max(topn, 1), np.float32)
    c = ctypes.c_int(0)
    rc = getattr(L, fn)(h, members.ctypes.data_as(ctypes.c_void_p), None if weights is None else weights.ctypes.data_as(ctypes.c_void_p),
                        k, None, 0, filt, topn, idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c))
    return rc, idx[:c.value].copy(), sc[:c.value].copy()


def test_null_weights_are_the_where_call(handle, engine_lib):
    from spotify_recommender_amd.engine import make_filter
    eng, feats = handle
    rows = np.array([5, 777, 12_345], np.int64)
    flt = make_filter(WHERE)
    for filt, where in ((None, None), (ctypes.byref(flt), WHERE)):
        rc, idx, sc = _raw(engine_lib, "mi355rec_query_playlist_topn_weighted", eng._h, rows, None, 3, 40, filt)
        assert rc == 0
        check((idx, sc), eng.query_playlist_topn(rows, 40, where=where), "NULL weights by row")
        vecs = np.ascontiguousarray(feats[rows])
        rc, idx, sc = _raw(engine_lib, "mi355rec_query_mean_topn_weighted", eng._h, vecs, None, 3, 40, filt)
        assert rc == 0
        check((idx, sc), eng.query_mean_topn(vecs, 40, where=where), "NULL weights by value")


def test_a_single_dislike_reverses_the_ranking(handle):
    eng, feats = handle
    for q in (0, 99, 12_345):
        c = oracle.scores(feats, feats[q])
        for topn in (200, 1024):
            idx, sc = eng.query_playlist_topn([q], topn, weights=[-1.0])
            check((idx, sc), expected_rows(feats, [q], [-1.0], [], topn), f"row {q}")
            assert np.array_equal(sc, -c[idx] + np.float32(0))                  # score = -c exactly
            ties = np.flatnonzero(np.diff(sc) == 0)
            assert np.all(np.diff(sc) <= 0) and np.all(idx[ties] < idx[ties + 1])
    idx, sc = eng.query_mean_topn(np.zeros((1, 12), np.float32), 30, weights=[-1.0])
    assert idx.tolist() == list(range(30)) and not sc.view(np.uint32).any()     # -0.0 reported as +0.0


def test_a_pair_that_cancels_scores_zero_everywhere(handle):
    eng, feats = handle
    a = 4242
    before = eng.playlist_counters()["rows_exact"]
    idx, sc = eng.query_playlist_topn([a, a], 50, weights=[1.0, -1.0])
    assert idx.tolist() == list(range(50)) and not sc.view(np.uint32).any()     # +0.0 each, rows ascending
    # |u| = 0: the pre-filter is off, every row took the chains
    assert eng.playlist_counters()["rows_exact"] - before == feats.shape[0]
    idx, sc = eng.query_mean_topn(feats[[a, a]], 1024, weights=[-3.0, 3.0])
    assert idx.tolist() == list(range(1024)) and not sc.view(np.uint32).any()
    # nearly cancelling: tiny |u|, scores of both signs
    w = [1.0, -1.0, 1e-3]
    check(eng.query_playlist_topn([a, a, 9], 100, weights=w), expected_rows(feats, [a, a, 9], w, [], 100), "nearly cancelling")


def test_zero_weight_and_zero_row_members(handle):
    eng, feats = handle
    a, b, z = 5, 777, 3000
    got = eng.query_playlist_topn([a, z, b], 60, weights=[1.0, 0.0, 0.5])
    check(got, expected_rows(feats, [a, z, b], [1.0, 0.0, 0.5], [], 60), "a zero-weight member")
    assert z not in got[0].tolist()
    without = eng.query_playlist_topn([a, b], 61, weights=[1.0, 0.5])[0].tolist()
    assert got[0].tolist() == [i for i in without if i != z][:60]
    got = eng.query_playlist_topn([a, b], 1024, weights=[1.0, -1.0])
    assert b not in got[0].tolist() and a not in got[0].tolist()                # a disliked member is excluded too
    for w in ([1.0, 2.0], [-1.0, 2.0], [1.0, -0.25]):
        check(eng.query_playlist_topn([10, a], 40, weights=w), expected_rows(feats, [10, a], w, [], 40), f"a zero row, {w}")
    check(eng.query_playlist_topn([10, 11], 40, weights=[1.0, -1.0]), expected_rows(feats, [10, 11], [1.0, -1.0], [], 40), "zero rows only")
    w = [1.0, -1.0, 0.75]                                                       # copies of row 99 that cancel exactly
    check(eng.query_playlist_topn([99, 100, 555], 64, weights=w), expected_rows(feats, [99, 100, 555], w, [], 64), "copies")


def test_counters_advance_and_the_prefilter_is_on_for_likes(big):
    eng, feats = big
    rng = np.random.default_rng(10)
    rows = rng.choice(N_BIG, size=10, replace=False)
    w = rng.uniform(0.25, 4.0, 10).astype(np.float32)
    before = eng.playlist_counters()
    eng.query_playlist_topn(rows, 10, weights=w)
    after = eng.playlist_counters()
    assert after["queries"] == before["queries"] + 1
    exact = after["rows_exact"] - before["rows_exact"]
    print(f"likes only, K=10, top-10 on {N_BIG} rows: rows_exact {exact}")
    assert 0 < exact < N_BIG, exact                                             # the pre-filter is on, not silently off
    # dislikes too (|u| stays well above 1e-3 here)
    wd = np.array([1.0] * 7 + [-0.5] * 3, np.float32)
    eng.query_playlist_topn(rows, 10, weights=wd)
    exact_d = eng.playlist_counters()["rows_exact"] - after["rows_exact"]
    print(f"7 likes + 3 dislikes at -0.5: rows_exact {exact_d}")
    assert 0 < exact_d < N_BIG, exact_d


def test_lane_answers_as_its_parent(big):
    eng, feats = big
    rows = [7, 70_000, 700_000, 7]
    w = [1.0, -0.5, 2.0, 0.25]
    want = eng.query_playlist_topn(rows, 200, [8, 9], where=WHERE, weights=w)
    check(want, expected_rows(feats, rows, w, [8, 9], 200, WHERE), "oracle")
    lane = eng.lane()
    try:
        check(lane.query_playlist_topn(rows, 200, [8, 9], where=WHERE, weights=w), want, "lane")
        check(lane.query_mean_topn(feats[rows], 200, weights=w), expected(feats, feats[rows], w, [], 200), "lane by value")
    finally:
        lane.close()


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = _special_rows(oracle.mt19937_uniform(9, 600_000))
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    rng = np.random.default_rng(9)
    with NodeEngine(feats, devices=[0, 0, 0], placement=pl) as node:
        for k in (1, 2, 7, 32):
            rows = rng.choice(600_000, size=k, replace=False)    # (on every virtual shard for k >= 7)
            excl = rng.integers(0, 600_000, size=1000)
            for kind, w in weight_kinds(rng, k):
                for topn in (1, 10, 1024):
                    what = f"{placement} k={k} {kind} top-{topn}"
                    check(node.query_playlist_topn(rows, topn, excl, weights=w), expected_rows(feats, rows, w, excl, topn), what + " by row")
                    check(node.query_mean_topn(feats[rows], topn, excl, where=WHERE, weights=w),
                          expected(feats, feats[rows], w, excl, topn, WHERE), what + " by value, filtered")
            ones = np.ones(k, np.float32)
            check(node.query_playlist_topn(rows, 100, excl, weights=ones), node.query_playlist_topn(rows, 100, excl), "weights of 1")
        check(node.query_playlist_topn([4242, 4242], 50, weights=[1.0, -1.0]),
              expected_rows(feats, [4242, 4242], [1.0, -1.0], [], 50), "cancelling")
        with pytest.raises(capi.Mi355Error) as e:
            node.query_playlist_topn([1, 2], 10, weights=[0.0, 0.0])
        assert e.value.code == capi.ERR_INVALID_ARG and "weights" in str(e.value)


def test_one_shard_node_forwards(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd.engine import NodeEngine
    feats = _special_rows(oracle.mt19937_uniform(12, 200_000))
    with NodeEngine(feats, devices=[0]) as node:
        rows, w = [3, 150_000, 77], [1.0, -0.5, 0.25]
        check(node.query_playlist_topn(rows, 100, [5], weights=w), expected_rows(feats, rows, w, [5], 100), "one shard by row")
        check(node.query_mean_topn(feats[rows], 100, weights=w), expected(feats, feats[rows], w, [], 100), "one shard by value")


def test_clustered_catalogue_likes_in_one_cluster_dislikes_in_another(engine_lib):
    import torch
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.synth import clustered_catalogue
    n, clusters = 2_000_000, 600
    t = clustered_catalogue(n, 0.03, seed=4242 + clusters, clusters=clusters, contiguous=True, ramp=False)
    feats = t.cpu().numpy()
    per = n // clusters
    rng = np.random.default_rng(600)
    liked = 17 * per + per // 4 + rng.choice(per // 2, size=7, replace=False)
    disliked = 401 * per + per // 4 + rng.choice(per // 2, size=3, replace=False)
    rows = np.concatenate([liked, disliked])
    with CosineEngine(t) as eng:
        for dw in (0.5, 1.0):
            w = np.array([1.0] * 7 + [-dw] * 3, np.float32)
            for topn in (100, 1024):
                check(eng.query_playlist_topn(rows, topn, weights=w), expected_rows(feats, rows, w, [], topn), f"-{dw} top-{topn}")
            check(eng.query_playlist_topn(rows, 100, [int(liked[0]) + 1], where={"tempo": (0.05, 0.95)}, weights=w),
                  expected_rows(feats, rows, w, [int(liked[0]) + 1], 100, {"tempo": (0.05, 0.95)}), "filtered")
        # dislikes only: the songs least like that cluster
        w = np.full(3, -1.0, np.float32)
        check(eng.query_playlist_topn(disliked, 100, weights=w), expected_rows(feats, disliked, w, [], 100), "dislikes only")
    del t
    torch.cuda.empty_cache()


def test_argument_errors(small, engine_lib):
    from spotify_recommender_amd import capi
    eng, feats = small
    ones2 = np.ones((2, 12), np.float32)
    bad_calls = [
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[1.0, np.nan]),
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[np.inf, 1.0]),
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[1.0, -np.inf]),
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[1.0, 1.5e6]),
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[-1.000001e6, 1.0]),
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[0.0, 0.0]),
        lambda: eng.query_playlist_topn([1, 2], 10, weights=[4e-7, -4e-7]),
        lambda: eng.query_mean_topn(ones2, 10, weights=[np.nan, 1.0]),
        lambda: eng.query_mean_topn(ones2, 10, weights=[0.0, -0.0]),
        lambda: eng.query_mean_topn(ones2, 10, weights=[2e6, 0.0]),
        lambda: eng.query_playlist_topn(list(range(33)), 10, weights=[1.0] * 33),
        lambda: eng.query_playlist_topn([1], 0, weights=[1.0]),
        lambda: eng.query_playlist_topn([1], 1025, weights=[1.0]),
        lambda: eng.query_playlist_topn([N_SMALL], 10, weights=[1.0]),
        lambda: eng.query_playlist_topn([1], 10, list(range(1025)), weights=[1.0]),
        lambda: eng.query_playlist_topn([1], 10, where={1: (0.9, 0.1)}, weights=[1.0]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(capi.Mi355Error) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARG, i
        assert str(e.value), i
    rows = np.array([1, 2], np.int64)
    for w in ([np.nan, 1.0], [0.0, 0.0], [1e7, 1.0]):
        for fn, members in (("mi355rec_query_playlist_topn_weighted", rows), ("mi355rec_query_mean_topn_weighted", ones2)):
            rc, _, _ = _raw(engine_lib, fn, eng._h, members, np.array(w, np.float32), 2, 10)
            assert rc == capi.ERR_INVALID_ARG
            assert b"weight" in engine_lib.mi355rec_last_error(eng._h)
    for w in ([1e6, -1e6], [1e-6, 0.0], [5e-7, -5e-7]):                         # the edges are allowed
        check(eng.query_playlist_topn([1, 2], 10, weights=w), expected_rows(feats, [1, 2], w, [], 10), f"edge {w}")
    check(eng.query_playlist_topn([1, 2], 10, weights=[1.0, -0.5]), expected_rows(feats, [1, 2], [1.0, -0.5], [], 10), "after errors")
