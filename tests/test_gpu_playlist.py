"""PLAYLISTS on the MI355X: the top-N by mean score against up to 32 songs (csrc/playlist.hip.h, playlist_scan_kernel: the
8-bit replica's pre-filter under the derived mean margin, K exact chains per surviving row) checked bit for bit against
the oracle (tests/playlist_oracle.py); K = 1 against the single-query routes; the exact path of small handles; hostile
values; lanes; node handles; the pre-filter's row count; single queries unchanged; the C++ drop-in."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import check
from tests.playlist_oracle import expected_from_scores, mean_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uniform_1m(engine_lib):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine
    feats = oracle.mt19937_uniform(77, 1_000_000)
    with CosineEngine(feats) as eng:
        yield eng, feats


@pytest.mark.parametrize("k", [1, 3, 10, 32])
def test_1m_uniform_matches_the_oracle(uniform_1m, k):
    eng, feats = uniform_1m
    rng = np.random.default_rng(k)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    scores = mean_scores(feats, feats[rows])
    excl = rng.integers(0, feats.shape[0], size=1000)
    # (the excluded list also holds rows of the true top: drawn from it, so the exclusion is exercised where it matters)
    top = expected_from_scores(scores, rows, 600)[0]
    excl[:300] = top[::2]
    for topn in (1, 100, 1024):
        check(eng.query_playlist_topn(rows, topn), expected_from_scores(scores, rows, topn), f"k={k} top-{topn}")
        check(eng.query_playlist_topn(rows, topn, excl), expected_from_scores(scores, list(rows) + excl.tolist(), topn),
              f"k={k} top-{topn} 1000 excluded")
        check(eng.query_mean_topn(feats[rows], topn, excl), expected_from_scores(scores, excl, topn), f"k={k} top-{topn} by value")
    vecs = rng.random((k, 12), dtype=np.float32)
    check(eng.query_mean_topn(vecs, 100), expected_from_scores(mean_scores(feats, vecs), [], 100), f"k={k} vectors")


def test_one_song_playlist_is_the_single_query(uniform_1m):
    eng, feats = uniform_1m
    for q in (0, 123_457, 999_999):
        for topn in (1, 100, 1024):
            got = eng.query_playlist_topn([q], topn)
            for want in (eng.query_row_topn(q, topn), eng.query_topn(feats[q], q, topn)):
                assert got[0].tolist() == want[0].tolist(), q
                assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), q
        got = eng.query_mean_topn(feats[q:q + 1], 100)
        want = eng.query_topn(feats[q], -1, 100)
        assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_prefilter_is_live(uniform_1m):
    eng, feats = uniform_1m
    rows = np.random.default_rng(10).choice(feats.shape[0], size=10, replace=False)
    before = eng.playlist_counters()
    eng.query_playlist_topn(rows, 10)
    after = eng.playlist_counters()
    assert after["queries"] == before["queries"] + 1
    exact = after["rows_exact"] - before["rows_exact"]
    # (at top-10: each workgroup's own threshold is the 10th best of the rows it has seen — DESIGN.md, PLAYLISTS)
    assert 0 < exact <= 0.05 * feats.shape[0], exact


def test_single_queries_unchanged_by_playlist_calls(uniform_1m):
    eng, feats = uniform_1m
    qs = (5, 500_000, 999_000)
    before = [eng.query_row_topn(q, 100) for q in qs]
    eng.query_playlist_topn([1, 2, 3, 4], 1024, list(range(100, 1100)))
    eng.query_mean_topn(np.zeros((2, 12), np.float32), 10)
    after = [eng.query_row_topn(q, 100) for q in qs]
    for (bi, bs), (ai, as_) in zip(before, after):
        assert bi.tolist() == ai.tolist() and np.array_equal(bs.view(np.uint32), as_.view(np.uint32))


def test_lane_answers_as_its_parent(uniform_1m):
    eng, feats = uniform_1m
    rows = [7, 70_000, 700_000, 7]
    want = eng.query_playlist_topn(rows, 200, [8, 9])
    lane = eng.lane()
    try:
        got = lane.query_playlist_topn(rows, 200, [8, 9])
        assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    finally:
        lane.close()


def test_10m_contiguous_clusters(engine_lib):
    import torch
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.synth import clustered_catalogue
    n, clusters = 10_000_000, 3000
    t = clustered_catalogue(n, 0.03, seed=4242 + clusters, clusters=clusters, contiguous=True, ramp=False)
    feats = t.cpu().numpy()
    per = n // clusters
    with CosineEngine(t) as eng:
        rng = np.random.default_rng(3000)
        for c in (17, 2999):
            rows = c * per + rng.choice(per, size=10, replace=False)
            scores = mean_scores(feats, feats[rows])
            for topn in (100, 1024):
                check(eng.query_playlist_topn(rows, topn), expected_from_scores(scores, rows, topn), f"cluster {c} top-{topn}")
    del t
    torch.cuda.empty_cache()


def test_exact_path_small_handles(engine_lib, golden_dir):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    feats = oracle.mt19937_uniform(5, 50_000)   # below the replica's 65 536 rows: every row exact
    with CosineEngine(feats) as eng:
        rng = np.random.default_rng(50)
        for k in (1, 4, 32):
            rows = rng.choice(50_000, size=k, replace=False)
            scores = mean_scores(feats, feats[rows])
            for topn in (1, 100, 1024):
                check(eng.query_playlist_topn(rows, topn, [0, 1, 2]), expected_from_scores(scores, list(rows) + [0, 1, 2], topn),
                      f"50k k={k} top-{topn}")
            before = eng.playlist_counters()["rows_exact"]
            eng.query_playlist_topn(rows, 10)
            assert eng.playlist_counters()["rows_exact"] - before == 50_000   # (no replica: the K chains for every row)
    g = np.load(golden_dir / "catalogue4096.npz")
    f = np.ascontiguousarray(g["feats"], dtype=np.float32)
    with CosineEngine(f) as eng:
        qs = [int(q) for q in g["queries"]][:8]
        check(eng.query_playlist_topn(qs, 50), expected_from_scores(mean_scores(f, f[qs]), qs, 50), "golden 4096")


N_HOSTILE = 700_003


def _hostile_catalogues():
    rng = np.random.default_rng(4)
    f = rng.random((N_HOSTILE, 12), dtype=np.float32)
    scale = (10.0 ** rng.uniform(-4.6, -3.4, size=N_HOSTILE)).astype(np.float32)   # |row| ~ 5e-5 .. 8e-4
    f *= scale[:, None]
    normal = rng.choice(N_HOSTILE, size=N_HOSTILE // 20, replace=False)
    f[normal] = rng.random((len(normal), 12), dtype=np.float32)
    yield "norm products straddling 1e-8", f
    rng = np.random.default_rng(5)
    f = rng.random((N_HOSTILE, 12), dtype=np.float32)
    vals = [np.nan, np.inf, -np.inf, 1e-42, 3e19, -3e19, 0.0]
    spots = rng.choice(N_HOSTILE, size=4000, replace=False)
    for i, r in enumerate(spots):
        f[r, rng.integers(0, 12)] = vals[i % len(vals)]
    big = np.zeros(12, dtype=np.float32)
    big[:3] = (3e19, 3e19, -3e19)
    f[spots[::4] + 1] = big
    yield "special rows", f
    rng = np.random.default_rng(3)
    f = (rng.normal(0, 1, size=(N_HOSTILE, 12)) * 10.0 ** rng.integers(-3, 4, size=(N_HOSTILE, 1))).astype(np.float32)
    yield "signed 1e-3..1e3", f


def test_hostile_values(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    for name, f in _hostile_catalogues():
        rng = np.random.default_rng(len(name))
        with CosineEngine(f) as eng:
            for k in (1, 5, 32):
                rows = rng.choice(N_HOSTILE, size=k, replace=False)
                scores = mean_scores(f, f[rows])
                check(eng.query_playlist_topn(rows, 100), expected_from_scores(scores, rows, 100), f"{name} k={k}")
            vecs = rng.random((6, 12), dtype=np.float32)
            vecs[:3] *= np.float32(1e-6)                                       # member norms outside the bound's range
            check(eng.query_mean_topn(vecs, 64), expected_from_scores(mean_scores(f, vecs), [], 64), f"{name} tiny members")
            vecs = rng.random((4, 12), dtype=np.float32)
            vecs[2:] = -vecs[:2]                                               # members that cancel: |u| = 0
            check(eng.query_mean_topn(vecs, 64), expected_from_scores(mean_scores(f, vecs), [], 64), f"{name} cancelling")
            big = np.zeros((2, 12), np.float32)
            big[:, :3] = (3e19, 3e19, -3e19)
            check(eng.query_mean_topn(big, 64), expected_from_scores(mean_scores(f, big), [], 64), f"{name} huge members")


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = oracle.mt19937_uniform(9, 600_000)
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    rng = np.random.default_rng(9)
    with CosineEngine(feats) as single, NodeEngine(feats, devices=[0, 0], placement=pl) as node:
        for k in (1, 6, 32):
            rows = rng.choice(600_000, size=k, replace=False)
            excl = rng.integers(0, 600_000, size=1000)
            for topn in (10, 1024):
                want = single.query_playlist_topn(rows, topn, excl)
                got = node.query_playlist_topn(rows, topn, excl)
                assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
                vecs = feats[rows]
                check(node.query_mean_topn(vecs, topn, excl), single.query_mean_topn(vecs, topn, excl), f"{placement} by value")
            check(want, expected_from_scores(mean_scores(feats, feats[rows]), list(rows) + excl.tolist(), 1024), "oracle")


def test_recommender_for_playlist_on_the_114k_csv(engine_lib, tmp_path):
    import torch  # noqa: F401
    from spotify_recommender_amd import build
    from tests.test_cpu_backend import _config1_csv
    build.build_shim()
    shim = ctypes.CDLL(str(build.LIB_SHIM))
    shim.shim_load.argtypes = [ctypes.c_char_p]
    shim.shim_load.restype = ctypes.c_void_p
    shim.shim_preprocess.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    for name in ("shim_free", "shim_initialize", "shim_is_gpu_enabled", "shim_get_song_count"):
        getattr(shim, name).argtypes = [ctypes.c_void_p]
    shim.shim_song_features.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    shim.shim_recommend_for_playlist.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    shim.shim_recommend_for_playlist.restype = ctypes.c_int64
    csv = tmp_path / "dataset.csv"
    _config1_csv(csv)
    out = tmp_path / "songs_data.bin"
    assert shim.shim_preprocess(str(csv).encode(), str(out).encode()) == 1
    h = shim.shim_load(str(out).encode())
    assert h
    try:
        assert shim.shim_initialize(h) == 1 and shim.shim_is_gpu_enabled(h) == 1
        n = 114_000
        feats = np.zeros((n, 12), np.float32)
        g = ctypes.c_int(0)
        for i in range(n):
            shim.shim_song_features(h, i, feats[i].ctypes.data, ctypes.byref(g))

        def rec(songs, topn, also=()):
            s = np.asarray(songs, np.int32)
            a = np.asarray(list(also) or [0], np.int32)
            res = np.full(topn, -1, np.int32)
            sc = np.zeros(topn, np.float32)
            c = shim.shim_recommend_for_playlist(h, s.ctypes.data, len(s), topn, a.ctypes.data, len(also), res.ctypes.data,
                                                 sc.ctypes.data, topn)
            return res[:max(c, 0)].astype(np.int64), sc[:max(c, 0)]

        songs = [0, 56_789, 113_999, 4_000]
        scores = mean_scores(feats, feats[songs])
        check(rec(songs, 10), expected_from_scores(scores, songs, 10), "recommendForPlaylist")
        also = [int(r) for r in expected_from_scores(scores, songs, 5)[0]]
        check(rec(songs, 10, also), expected_from_scores(scores, songs + also, 10), "alsoExclude")
        assert rec([], 10)[0].size == 0 and rec([n], 10)[0].size == 0 and rec(songs, 0)[0].size == 0
    finally:
        shim.shim_free(h)
