"""The BUCKETED cutoff sample of the 8-bit scan (csrc/replica_q8.hip.h, "the bucketed sample"; mi355rec_set_sample): the structure a
handle builds beside its replica, and queries that take their launch-wide bound from it, against the oracle — ids and scores bit
for bit (oracle.topn_canonical).

The sample only places the bound; what can go wrong is a stored value that is not the exact score of a real, distinct, eligible
row (duplicates of the query, marker rows, the excluded row, padding) — then the top-N loses rows.  The structure exists where
the 8-bit scan takes exact sample values: from 1025 tiles of 2048 rows up on a device whose scan keeps 512 workgroups resident,
so 2 097 153 rows is the smallest catalogue used here."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

N_MIN = 2_097_153          # the smallest shard with the structure: % 2048 == 1
REGION = 2048


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def Engine(torch_cuda):
    from spotify_recommender_amd.engine import CosineEngine
    return CosineEngine


@pytest.fixture(scope="module")
def capi():
    from spotify_recommender_amd import capi
    return capi


@pytest.fixture(scope="module")
def uniform():
    """One uniform catalogue of N_MIN rows, shared and left unchanged."""
    f = np.random.default_rng(41).random((N_MIN, 12), dtype=np.float32)
    f.setflags(write=False)
    return f


def check(f, got, q, excl, topn, what):
    idx, sc = got
    want_i, want_s = oracle.topn_canonical(oracle.scores(f, np.ascontiguousarray(q, dtype=np.float32), threads=0), int(excl), topn)
    assert np.asarray(idx).tolist() == want_i.tolist(), what
    assert np.array_equal(np.asarray(sc, dtype=np.float32).view(np.uint32), (want_s + np.float32(0)).view(np.uint32)), what


def bucketed(eng, capi):
    eng.set_sample(capi.SAMPLE_BUCKETED)
    return eng


# ---- the structure --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_MIN, 2_359_299])
def test_structure(Engine, capi, uniform, n):
    f = uniform if n == N_MIN else np.random.default_rng(n).random((n, 12), dtype=np.float32)
    with Engine(f) as eng:
        info = eng.bucket_sample_info()
        regions = min(1024, n // (5 * REGION))
        assert info["regions"] == regions == info["centroids"] and info["base_rows"] == regions * REGION, info
        assert info["picks"] == 32 and info["bytes"] == regions * REGION * 16 + regions * 48 + regions * 8 and info["build_ms"] > 0, info
        stride = info["stride_rows"]
        assert stride == (n // regions) // 4 * 4 and stride >= REGION
        rows, tab = eng.bucket_sample_rows()
        # a duplicate-free subset of [0, n) that equals the strided base as a set
        assert rows.min() >= 0 and rows.max() < n and np.unique(rows).size == rows.size
        base = (np.arange(regions, dtype=np.int64)[:, None] * stride + np.arange(REGION)[None, :]).ravel()
        assert np.array_equal(np.sort(rows.astype(np.int64)), base)
        # the region table: ordered, and every entry's bucket range holds a centroid that is (to fp32 rounding: 12 products of
        # magnitude <= sqrt(12), 2^-24 each) as near to the row as any centroid
        assert np.all(tab[:, 0] <= tab[:, 1]) and np.all(tab[1:, 0] >= tab[:-1, 1]) and tab.min() >= 0 and tab.max() < regions
        cs = info["centroid_stride"]
        assert cs == n // regions
        cent = f[np.arange(regions, dtype=np.int64) * cs + cs // 2].astype(np.float64)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
        for g in range(0, regions, max(1, regions // 48)):   # (a spread of regions, the first and the last included below)
            for gg in {g, regions - 1}:
                dots = f[rows[gg * REGION:(gg + 1) * REGION]].astype(np.float64) @ cent.T
                in_range = dots[:, tab[gg, 0]:tab[gg, 1] + 1].max(axis=1)
                assert np.all(in_range >= dots.max(axis=1) - 1e-5), gg
        # rows inside a bucket ascend: a descent only where the bucket changes, so at most regions - 1 of them
        assert np.count_nonzero(np.diff(rows) < 0) <= regions - 1
        eng.set_sample(capi.SAMPLE_BUCKETED)
        assert eng.bucket_sample_info()["mode"] == capi.SAMPLE_BUCKETED


def test_no_structure_below_the_exact_sample(Engine, capi):
    f = np.random.default_rng(3).random((300_001, 12), dtype=np.float32)
    with Engine(f) as eng:
        eng.set_replica(capi.REPLICA_ON)
        assert eng.bucket_sample_info()["base_rows"] == 0
        with pytest.raises(Exception):
            eng.set_sample(capi.SAMPLE_BUCKETED)
        with pytest.raises(Exception):
            eng.set_sample(7)
        eng.set_sample(capi.SAMPLE_STRIDED)
        eng.set_sample(capi.SAMPLE_AUTO)
        check(f, eng.query_row_topn(5, 100), f[5], 5, 100, "small shard")
        assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_STRIDED


# ---- values that must be exact scores of distinct eligible rows ---------------------------------------------------------
def test_ties_and_distinctness(Engine, capi):
    """1000 copies of the query row: a sample that counted one row twice, or the excluded row, would place the bound at the
    copies' score with fewer than topn rows behind it."""
    rng = np.random.default_rng(17)
    n = N_MIN
    f = rng.random((n, 12), dtype=np.float32)
    qrow = 1_234_567
    copies = rng.choice(n, size=1000, replace=False)
    f[copies] = f[qrow]
    with Engine(f) as eng:
        bucketed(eng, capi)
        before = eng.replica_counters()
        for topn in (1, 100, 128):
            check(f, eng.query_row_topn(qrow, topn), f[qrow], qrow, topn, f"by row, top-{topn}")
            check(f, eng.query_topn(f[qrow], -1, topn), f[qrow], -1, topn, f"by value, top-{topn}")
            check(f, eng.query_row_topn(int(copies[3]), topn), f[qrow], int(copies[3]), topn, f"a copy by row, top-{topn}")
        assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_BUCKETED
        assert eng.replica_counters()["scans"] - before["scans"] == 9


def test_ineligible_rows_in_the_best_regions(Engine, capi):
    """A clustered catalogue whose rows nearest the query are NaN / huge / tiny (marker rows of the replica) or exactly zero: none of
    them may give a sample value, all of them go to the exact chain."""
    rng = np.random.default_rng(23)
    n = N_MIN
    centres = rng.random((64, 12), dtype=np.float32)
    f = (centres[rng.integers(0, 64, size=n)] + rng.normal(0, 0.02, (n, 12)).astype(np.float32)).astype(np.float32)
    q = (centres[5] + np.float32(0.01)).astype(np.float32)
    near = np.argsort(-oracle.scores(f, q, threads=0), kind="stable")[:4000]
    f[near[0::4]] = np.nan
    f[near[1::4]] *= np.float32(1e30)
    f[near[2::4]] *= np.float32(1e-30)
    f[near[3::4]] = 0
    with Engine(f) as eng:
        bucketed(eng, capi)
        before = eng.replica_counters()
        for topn in (10, 100):
            check(f, eng.query_topn(q, -1, topn), q, -1, topn, f"top-{topn}")
        after = eng.replica_counters()
        # the 3000 marker rows are re-scored by every scan
        assert after["rescored_rows"] - before["rescored_rows"] >= 2 * 3000
        # ... and a query with nothing hostile near it
        check(f, eng.query_topn(centres[40], -1, 100), centres[40], -1, 100, "another cluster")


def test_excluded_row_is_the_best_of_its_group(Engine, capi, uniform):
    f = uniform
    with Engine(f) as eng:
        bucketed(eng, capi)
        rows, _ = eng.bucket_sample_rows()
        for r in (int(rows[0]), int(rows[REGION * 7 + 63]), int(rows[-1])):   # base rows: each scores 1.0 against itself
            check(f, eng.query_row_topn(r, 100), f[r], r, 100, f"row {r}")
            check(f, eng.query_topn(f[r], r, 100), f[r], r, 100, f"row {r} by value")


def test_excluded_row_far_from_every_other_row(Engine, capi, uniform):
    """A case the exclusion test decides: base row r points away from every other row (all cosines against it are negative), so
    r's own 1.0 is the only sample value anywhere near the top.  Were it stored, the top-1 bound would be 1.0 and the cutoff
    (1.0 - margin) above every eligible row: an empty or wrong top-1."""
    f = np.array(uniform)
    n = f.shape[0]
    regions = min(1024, n // (5 * REGION))
    stride = (n // regions) // 4 * 4
    r = 5 * stride + 100                      # a row of the strided base
    f[r] = -np.random.default_rng(9).random(12, dtype=np.float32) - np.float32(0.1)
    with Engine(f) as eng:
        bucketed(eng, capi)
        rows, _ = eng.bucket_sample_rows()
        assert r in set(rows[:].tolist())
        for topn in (1, 2, 10):
            check(f, eng.query_row_topn(r, topn), f[r], r, topn, f"by row, top-{topn}")
            check(f, eng.query_topn(f[r], r, topn), f[r], r, topn, f"by value, top-{topn}")
        # ... streamed: the riders of the launch before take the sample
        import torch
        from spotify_recommender_amd.engine import unpack_keys
        out = torch.zeros((3, 1), dtype=torch.int64, device="cuda:0")
        for i, row in enumerate((7, r, r)):
            eng.enqueue_row_keys_streamed(int(row), 1, out[i])
        eng.enqueue_flush()
        torch.cuda.synchronize()
        for i, row in enumerate((7, r, r)):
            check(f, unpack_keys(out[i].cpu().numpy()), f[row], int(row), 1, f"streamed {i}")
        assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_BUCKETED


# ---- shape edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025 * 2048, N_MIN, 1027 * 2048 - 1])   # n % 2048 in {0, 1, 2047}
def test_shape_edges(Engine, capi, uniform, n):
    f = uniform if n == N_MIN else np.random.default_rng(n).random((n, 12), dtype=np.float32)
    with Engine(f) as eng:
        assert eng.bucket_sample_info()["base_rows"] > 0
        bucketed(eng, capi)
        for k, topn in enumerate((1, 100, 128, 129, 1024)):
            r = (n - 1, 0, n // 2, n - 2, 77)[k]
            check(f, eng.query_row_topn(r, topn), f[r], r, topn, f"n {n} top-{topn}")
            assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_BUCKETED


# ---- streams ----------------------------------------------------------------------------------------------------------------
def _stream(torch, pair, streams, qrows, topn, toggle=None, flush_at=None):
    from spotify_recommender_amd.engine import unpack_keys
    outs = [torch.zeros(topn, dtype=torch.int64, device="cuda:0") for _ in qrows]
    torch.cuda.synchronize()
    for k, (o, r) in enumerate(zip(outs, qrows)):
        if toggle is not None:
            pair[k % 2].set_sample(toggle[(k // 2) % len(toggle)])
        pair[k % 2].enqueue_row_keys_streamed(int(r), topn, o, stream=streams[k % 2])
        if flush_at is not None and k == flush_at:
            for ln, ls in zip(pair, streams):
                ln.enqueue_flush(stream=ls)
    for ln, ls in zip(pair, streams):
        ln.enqueue_flush(stream=ls)
    torch.cuda.synchronize()
    return [unpack_keys(o.cpu().numpy()) for o in outs]


def test_streams_over_two_lanes(Engine, capi, torch_cuda, uniform):
    torch = torch_cuda
    f = uniform
    qrows = np.random.default_rng(5).integers(0, f.shape[0], size=64)
    with Engine(f) as eng:
        bucketed(eng, capi)
        sync = [eng.query_row_topn(int(r), 100) for r in qrows]
        for r, got in list(zip(qrows, sync))[:8]:
            check(f, got, f[r], int(r), 100, f"sync row {r}")
        lane = eng.lane()
        pair, streams = [eng, lane], [eng.own_stream(), lane.own_stream()]
        try:
            lane.set_sample(capi.SAMPLE_BUCKETED)
            got = _stream(torch, pair, streams, qrows, 100, flush_at=31)
            assert lane.bucket_sample_info()["last_used"] == capi.SAMPLE_BUCKETED
            for k, ((gi, gs), (wi, ws)) in enumerate(zip(got, sync)):
                assert gi.tolist() == wi.tolist() and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"streamed query {k}"
            # the same with the sample toggled between queries: every query's sample is its own
            modes = (capi.SAMPLE_STRIDED, capi.SAMPLE_BUCKETED, capi.SAMPLE_BUCKETED, capi.SAMPLE_AUTO, capi.SAMPLE_STRIDED)
            got = _stream(torch, pair, streams, qrows, 100, toggle=modes, flush_at=30)
            for k, ((gi, gs), (wi, ws)) in enumerate(zip(got, sync)):
                assert gi.tolist() == wi.tolist() and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"toggled query {k}"
        finally:
            lane.close()


def test_rebuild_after_rows_changed_in_place(Engine, capi, torch_cuda, uniform):
    torch = torch_cuda
    f = np.array(uniform)
    dev = torch.from_numpy(f).to("cuda:0")
    with Engine(dev) as eng:
        bucketed(eng, capi)
        check(f, eng.query_row_topn(1000, 100), f[1000], 1000, 100, "before")
        old_rows, _ = eng.bucket_sample_rows()
        f2 = np.random.default_rng(77).random(f.shape, dtype=np.float32)
        dev.copy_(torch.from_numpy(f2))
        torch.cuda.synchronize()
        eng.rebuild_replica()
        info = eng.bucket_sample_info()
        assert info["base_rows"] == old_rows.size and info["mode"] == capi.SAMPLE_BUCKETED
        new_rows, _ = eng.bucket_sample_rows()
        assert not np.array_equal(new_rows, old_rows) and np.array_equal(np.sort(new_rows), np.sort(old_rows))
        for r in (1000, int(new_rows[5])):
            check(f2, eng.query_row_topn(r, 100), f2[r], r, 100, f"after the rebuild, row {r}")
        out = torch.zeros((4, 100), dtype=torch.int64, device="cuda:0")
        for i in range(4):
            eng.enqueue_row_keys_streamed(10 + i, 100, out[i])
        eng.enqueue_flush()
        torch.cuda.synchronize()
        from spotify_recommender_amd.engine import unpack_keys
        for i in range(4):
            check(f2, unpack_keys(out[i].cpu().numpy()), f2[10 + i], 10 + i, 100, f"streamed after the rebuild {i}")


# ---- AUTO ---------------------------------------------------------------------------------------------------------------
def test_auto_just_above_its_threshold(Engine, capi, torch_cuda):
    """AUTO takes the bucketed sample for topn <= 128 from capi.SAMPLE_AUTO_MIN_ROWS rows up (6 M: the row count from which it
    measured no slower than the strided one at top-10 and top-100); its bound is tighter than the strided sample's there (measured
    0.76x the candidates at 6 M rows; a CPU model of both gives 0.95-1.1x at 3.2-4 M and 0.55x at 10 M): at most 1.5x the rows
    re-scored, so that a sample that silently yields no bound cannot pass."""
    torch = torch_cuda
    n = capi.SAMPLE_AUTO_MIN_ROWS + 3
    rng = np.random.default_rng(31)
    f = rng.random((n, 12), dtype=np.float32)
    qrows = rng.integers(0, n, size=32)
    with Engine(f) as eng:
        assert eng.bucket_sample_info()["mode"] == capi.SAMPLE_AUTO
        out = torch.zeros((32, 100), dtype=torch.int64, device="cuda:0")

        def stream():
            before = eng.replica_counters()["rescored_rows"]
            for i, r in enumerate(qrows):
                eng.enqueue_row_keys_streamed(int(r), 100, out[i])
            eng.enqueue_flush()
            torch.cuda.synchronize()
            return (eng.replica_counters()["rescored_rows"] - before) / len(qrows)

        per_auto = stream()
        assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_BUCKETED
        from spotify_recommender_amd.engine import unpack_keys
        for i, r in enumerate(qrows):
            check(f, unpack_keys(out[i].cpu().numpy()), f[r], int(r), 100, f"AUTO query {i}")
        def pair_streamed(topn):   # two streamed queries: the second one's sample rides in the first one's launch
            keys = torch.zeros((2, topn), dtype=torch.int64, device="cuda:0")
            for i in range(2):
                eng.enqueue_row_keys_streamed(int(qrows[i]), topn, keys[i])
            used = eng.bucket_sample_info()["last_used"]
            eng.enqueue_flush()
            torch.cuda.synchronize()
            for i in range(2):
                check(f, unpack_keys(keys[i].cpu().numpy()), f[qrows[i]], int(qrows[i]), topn, f"streamed top-{topn} query {i}")
            return used

        for topn in (129, 1024):   # beyond what was modelled: the strided sample
            assert pair_streamed(topn) == capi.SAMPLE_STRIDED
        assert pair_streamed(128) == capi.SAMPLE_BUCKETED
        # a query alone has a sample launch of its own, on its critical path: the strided sample under AUTO
        check(f, eng.query_row_topn(int(qrows[1]), 100), f[qrows[1]], int(qrows[1]), 100, "alone, top-100")
        assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_STRIDED
        eng.set_sample(capi.SAMPLE_STRIDED)
        per_strided = stream()
        print(f"rescored rows per query at {n} rows, top-100: AUTO (bucketed) {per_auto:.0f}, strided {per_strided:.0f}")
        assert 0 < per_auto <= 1.5 * per_strided, (per_auto, per_strided)
