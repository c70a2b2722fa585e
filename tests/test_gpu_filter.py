"""FEATURE FILTERS on the MI355X: the filtered playlist calls (csrc/playlist.hip.h, playlist_scan_kernel: the predicate on
each fp32 row read, before the K chains) checked bit for bit against the oracle (tests/filter_oracle.py) over pass rates
from all rows to none; K = 1 against the single-query routes; the pre-filter still live; the exact path of small handles;
hostile values; lanes; node handles; unfiltered calls unchanged; a 10 M clustered catalogue; the C++ drop-in."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.filter_oracle import expected_where, pass_mask
from tests.labels_oracle import check
from tests.playlist_oracle import mean_scores

pytestmark = pytest.mark.gpu

# one constrained feature (key, column 2) of a uniform catalogue: the pass rate is known from the data
RATES = {"all": {2: (0.0, 1.0)}, "half": {2: (0.25, 0.75)}, "5pct": {"key": (0.40, 0.45)}, "0.1pct": {2: (0.9, 0.901)},
         "none": {2: (1.5, 2.0)}}


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
    rng = np.random.default_rng(100 + k)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    scores = mean_scores(feats, feats[rows])
    for rname, where in RATES.items():
        rate = pass_mask(feats, where).mean()
        excl = rng.integers(0, feats.shape[0], size=1000)
        top = expected_where(scores, feats, where, rows, 600)[0]
        excl[:min(300, top.size)] = top[::2][:300]     # drawn from the true (filtered) top
        for topn in (1, 100, 1024):
            what = f"k={k} {rname} ({rate:.4f}) top-{topn}"
            check(eng.query_playlist_topn(rows, topn, where=where), expected_where(scores, feats, where, rows, topn), what)
            check(eng.query_playlist_topn(rows, topn, excl, where=where),
                  expected_where(scores, feats, where, list(rows) + excl.tolist(), topn), what + " 1000 excluded")
            check(eng.query_mean_topn(feats[rows], topn, excl, where=where), expected_where(scores, feats, where, excl, topn),
                  what + " by value")


def test_all_pass_single_query_is_the_single_query(uniform_1m):
    eng, feats = uniform_1m
    for q in (0, 123_457, 999_999):
        for topn in (1, 100, 1024):
            got = eng.query_playlist_topn([q], topn, where={"energy": (-np.inf, np.inf)})
            for want in (eng.query_row_topn(q, topn), eng.query_topn(feats[q], q, topn)):
                check(got, want, f"row {q} top-{topn}")
        got = eng.query_mean_topn(feats[q:q + 1], 100, where={0: (0.0, 1.0)})
        check(got, eng.query_topn(feats[q], -1, 100), f"by value {q}")
        check(eng.query_playlist_topn([q], 100, where={}), eng.query_row_topn(q, 100), f"active == 0, row {q}")


def test_prefilter_stays_live_under_a_permissive_filter(uniform_1m):
    eng, feats = uniform_1m
    rows = np.random.default_rng(10).choice(feats.shape[0], size=10, replace=False)
    before = eng.playlist_counters()
    eng.query_playlist_topn(rows, 10, where={"key": (0.0, 0.9)})
    after = eng.playlist_counters()
    assert after["queries"] == before["queries"] + 1
    read = after["rows_exact"] - before["rows_exact"]
    assert 0 < read <= 0.05 * feats.shape[0], read


def test_unfiltered_calls_unchanged_by_filtered_ones(uniform_1m):
    eng, feats = uniform_1m
    qs = (5, 500_000, 999_000)
    single = [eng.query_row_topn(q, 100) for q in qs]
    lists = [eng.query_playlist_topn([q, q + 1, q + 2], 100, [q + 3]) for q in qs]
    for rname, where in RATES.items():
        eng.query_playlist_topn([1, 2, 3, 4], 1024, list(range(100, 1100)), where=where)
        eng.query_mean_topn(np.zeros((2, 12), np.float32), 10, where=where)
    for q, want in zip(qs, single):
        check(eng.query_row_topn(q, 100), want, f"single {q}")
    for q, want in zip(qs, lists):
        check(eng.query_playlist_topn([q, q + 1, q + 2], 100, [q + 3]), want, f"playlist {q}")


def test_lane_answers_as_its_parent(uniform_1m):
    eng, feats = uniform_1m
    rows = [7, 70_000, 700_000, 7]
    where = {2: (0.3, 0.6), "liveness": (0.0, 0.5)}
    want = eng.query_playlist_topn(rows, 200, [8, 9], where=where)
    lane = eng.lane()
    try:
        check(lane.query_playlist_topn(rows, 200, [8, 9], where=where), want, "lane")
    finally:
        lane.close()
    check(want, expected_where(mean_scores(feats, feats[rows]), feats, where, rows + [8, 9], 200), "oracle")


def test_exact_path_small_handles(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    feats = oracle.mt19937_uniform(5, 50_000)   # below the replica's 65 536 rows: every row read exactly
    with CosineEngine(feats) as eng:
        rng = np.random.default_rng(50)
        for k in (1, 4, 32):
            rows = rng.choice(50_000, size=k, replace=False)
            scores = mean_scores(feats, feats[rows])
            for rname in ("all", "5pct", "0.1pct", "none"):
                for topn in (1, 100, 1024):
                    check(eng.query_playlist_topn(rows, topn, [0, 1, 2], where=RATES[rname]),
                          expected_where(scores, feats, RATES[rname], list(rows) + [0, 1, 2], topn), f"50k k={k} {rname} top-{topn}")
            before = eng.playlist_counters()["rows_exact"]
            eng.query_playlist_topn(rows, 10, where=RATES["5pct"])
            assert eng.playlist_counters()["rows_exact"] - before == 50_000   # (every row read, rejected ones included)


def test_hostile_values(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    from tests.test_gpu_playlist import N_HOSTILE, _hostile_catalogues
    wheres = [{0: (-np.inf, np.inf), 5: (-np.inf, np.inf)},   # NaN features fail; every other value passes
              {1: (0.0, 1e20)}, {3: (-np.inf, 0.0)}, {4: (0.0, 0.0)}, {6: (0.2, 0.4), 7: (-1e30, 0.9)}]
    for name, f in _hostile_catalogues():
        rng = np.random.default_rng(len(name))
        with CosineEngine(f) as eng:
            for k in (1, 5, 32):
                rows = rng.choice(N_HOSTILE, size=k, replace=False)
                scores = mean_scores(f, f[rows])
                for i, where in enumerate(wheres):
                    check(eng.query_playlist_topn(rows, 100, where=where), expected_where(scores, f, where, rows, 100),
                          f"{name} k={k} filter {i}")
            vecs = rng.random((4, 12), dtype=np.float32)
            vecs[2:] = -vecs[:2]                                               # members that cancel: the pre-filter is off
            check(eng.query_mean_topn(vecs, 64, where=wheres[4]), expected_where(mean_scores(f, vecs), f, wheres[4], [], 64),
                  f"{name} cancelling")


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
            for where in (RATES["half"], RATES["0.1pct"]):
                for topn in (10, 1024):
                    want = single.query_playlist_topn(rows, topn, excl, where=where)
                    check(node.query_playlist_topn(rows, topn, excl, where=where), want, f"{placement} by row")
                    vecs = feats[rows]
                    check(node.query_mean_topn(vecs, topn, excl, where=where), single.query_mean_topn(vecs, topn, excl, where=where),
                          f"{placement} by value")
                check(want, expected_where(mean_scores(feats, feats[rows]), feats, where, list(rows) + excl.tolist(), 1024), "oracle")


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
        rows = 17 * per + rng.choice(per, size=10, replace=False)
        scores = mean_scores(feats, feats[rows])
        lo = float(np.median(feats[rows, 1]))
        where = {1: (lo, 1.0), "tempo": (0.1, 0.9)}    # about half of the members' cluster
        for topn in (100, 1024):
            check(eng.query_playlist_topn(rows, topn, where=where), expected_where(scores, feats, where, rows, topn), f"top-{topn}")
    del t
    torch.cuda.empty_cache()


def test_recommend_by_index_where_on_the_114k_csv(engine_lib, tmp_path):
    import torch  # noqa: F401
    from spotify_recommender_amd import build
    from tests.test_cpu_backend import _config1_csv
    build.build_shim()
    shim = ctypes.CDLL(str(build.LIB_SHIM))
    shim.shim_load.argtypes = [ctypes.c_char_p]
    shim.shim_load.restype = ctypes.c_void_p
    shim.shim_preprocess.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    for name in ("shim_free", "shim_initialize", "shim_is_gpu_enabled"):
        getattr(shim, name).argtypes = [ctypes.c_void_p]
    shim.shim_song_features.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    shim.shim_recommend_by_index_where.restype = ctypes.c_int64
    shim.shim_recommend_by_index_where.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
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

        def rec(idx, topn, ranges):
            f = np.array([r[0] for r in ranges] or [0], np.int32)
            lo = np.array([r[1] for r in ranges] or [0], np.float32)
            hi = np.array([r[2] for r in ranges] or [0], np.float32)
            res = np.full(topn, -1, np.int32)
            sc = np.zeros(topn, np.float32)
            c = shim.shim_recommend_by_index_where(h, idx, topn, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(ranges),
                                                   res.ctypes.data, sc.ctypes.data, topn)
            return res[:max(c, 0)].astype(np.int64), sc[:max(c, 0)]

        for q in (0, 56_789, 113_999):
            scores = oracle.scores(feats, feats[q])
            for ranges, where in (([(1, 0.7, 1.0)], {1: (0.7, 1.0)}),                         # high energy
                                  ([(8, 0.0, 0.3), (1, 0.2, 0.9), (1, 0.5, 1.0)], {8: (0.0, 0.3), 1: (0.5, 0.9)})):
                check(rec(q, 10, ranges), expected_where(scores, feats, where, [q], 10), f"song {q}")
        assert rec(5, 10, [(12, 0.0, 1.0)])[0].size == 0 and rec(5, 10, [(1, 0.5, 0.4)])[0].size == 0
    finally:
        shim.shim_free(h)
