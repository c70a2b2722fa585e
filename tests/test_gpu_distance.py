"""DISTANCE REQUESTS on the MI355X (csrc/playlist.hip.h, "DISTANCE": the distance branch of playlist_scan_kernel, its per-row
cut over the 8-bit replica and the norms q8_build_kernel leaves), through mi355rec_query_distance_request and its node-handle
twin, bit for bit against tests/distance_oracle.py: ids, distance bits, counts and padding, no tolerances.  Sizes at the quad,
the 2048-row tile, kPlBoundRows, the 4096-row anchor table and several workgroups; without a replica (every row takes the
chains) and with one (the pre-filter); one 1 M-row catalogue on which many workgroups publish thresholds to each other.

Which copy the scan reads: the 8-bit replica whenever the handle HAS one, so "replica off" is a handle that never built one
and "replica on" one that did (set_replica(ON) builds it on demand), as in tests/test_gpu_prior.py."""
import numpy as np
import pytest

from oracle import oracle
from tests.distance_oracle import check, expected_from_m, hostile_catalogue, mean_sqdist, request_call
from tests.labels_oracle import check as check_scores
from tests.playlist_labels_oracle import uniform_labels

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 4, 5, 257, 2047, 2048, 2049, 4097, 65_537]
TOPNS = (1, 10, 256, 257, 1024)
N_BIG = 1_000_003


def _call(eng, **kw):
    from spotify_recommender_amd import capi
    rc, ids, dist = request_call(capi, eng._lib.mi355rec_query_distance_request, eng._h, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, dist


def _engines(feats):
    """("replica off", engine) then ("replica on", engine), one alive at a time."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA if feats.shape[0] >= 65_536 else 0) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


def _member_cases(rng, feats):
    """[(k, rows, vecs, m by row, m by value)]: the oracle's m once per set of members."""
    n = feats.shape[0]
    out = []
    for k in sorted({min(k, n) for k in (1, 3, 32)}):
        rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = np.nan_to_num(feats[int(rng.integers(0, n))], nan=0.5, posinf=1.0, neginf=-1.0)
        out.append((k, rows, vecs, mean_sqdist(feats, feats[rows]), mean_sqdist(feats, vecs)))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    feats = oracle.mt19937_uniform(700 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    cases = _member_cases(rng, feats)
    results = {}
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        for k, rows, vecs, m_r, m_v in cases:
            for topn in TOPNS:
                what = f"n={n} [{mode}] K={k} top-{topn}"
                got = _call(eng, rows=rows, topn=topn)
                check(got, expected_from_m(feats, m_r, rows, topn), what + " by row")
                results.setdefault((k, topn), []).append(got)
                check(_call(eng, members=vecs, topn=topn), expected_from_m(feats, m_v, [], topn), what + " by value")
                check(_call(eng, members=vecs, exclude=[n - 1, 0, 0], where=WHERE, labels=WANTED, topn=topn),
                      expected_from_m(feats, m_v, [n - 1, 0], topn, WHERE, lab, WANTED), what + " composed")
    for key, (off, on) in results.items():                        # replica on and off: identical results
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [5, 257, 4097, 70_001])
def test_hostile_rows_and_members(engine_lib, n):
    """NaN, +-inf, all-zero, 1e-30 and 1e30 rows, duplicates; members that are tiny, zero or not finite."""
    feats = hostile_catalogue(n)
    rng = np.random.default_rng([9, n])
    for mode, eng in _engines(feats):
        for k in (1, 3, 32):
            rows = [0] + [int(r) for r in rng.choice(np.arange(1, n), size=min(k, n) - 1, replace=False)]   # hostile rows among them
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            tiny = vecs.copy()
            tiny[k // 2] = np.float32(1e-30)
            zero = np.zeros((k, 12), np.float32)
            for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []), ("by row", dict(rows=rows), feats[rows], rows),
                                                ("tiny member", dict(members=tiny), tiny, []), ("zero members", dict(members=zero), zero, [])):
                m = mean_sqdist(feats, members)
                n_adm = int(expected_from_m(feats, m, excluded, n)[0].size)
                for topn in sorted({1, 10, 257, 1024, max(1, min(1024, n_adm)), min(1024, n_adm + 1)}):
                    got = _call(eng, topn=topn, **kw)
                    check(got, expected_from_m(feats, m, excluded, topn), f"hostile n={n} [{mode}] K={k} {what} top-{topn}")
                    assert got[0].size == min(topn, n_adm)
            for bad_value in (np.nan, np.inf, -np.inf, 1e30):    # no row has a finite m: nothing is listed
                bad = vecs.copy()
                bad[k - 1, 5] = bad_value
                assert _call(eng, members=bad, topn=10)[0].size == 0, (mode, k, bad_value)
        # the duplicates of row 0 come first, by row, at distance +0.0f
        dups = [i for i in range(n) if np.array_equal(feats[i], feats[0])]
        ids, dist = _call(eng, members=feats[:1], topn=len(dups))
        assert ids.tolist() == dups and not dist.view(np.uint32).any()


@pytest.fixture(scope="module")
def big(engine_lib):
    """(feats, member vector, m of every row): computed once, never modified."""
    feats = oracle.mt19937_uniform(2026, N_BIG)
    q = feats[123_457].copy()
    return feats, q, mean_sqdist(feats, q[None, :])


def test_1m_rows_many_workgroups_and_the_prefilter_works(big):
    """Top-10 of 1 M uniform rows, k = 1: the oracle's answer, and rows_exact: at most n / 4 with the replica (the model gives
    well under 1 % at the true threshold; the anchors' start is looser), exactly the rows read without it."""
    feats, q, m = big
    for mode, eng in _engines(feats):
        before = eng.playlist_counters()
        got = _call(eng, members=q, topn=10)
        after = eng.playlist_counters()
        exact = after["rows_exact"] - before["rows_exact"]
        print(f"[{mode}] rows_exact {exact} of {N_BIG} ({100.0 * exact / N_BIG:.3f} %)")
        check(got, expected_from_m(feats, m, [], 10), f"1 M rows [{mode}]")
        assert after["queries"] - before["queries"] == 1
        if mode == "replica on":
            assert 0 < exact <= N_BIG // 4, exact
            got = _call(eng, rows=[123_457], exclude=[5, 6], where=WHERE, topn=100)     # the other shapes on many workgroups
            check(got, expected_from_m(feats, m, [123_457, 5, 6], 100, WHERE), "1 M rows, by row, composed")
        else:
            assert exact == N_BIG, exact


def test_lanes_interleaving_and_rebuild(engine_lib):
    """A lane gives its parent's results; cosine playlist requests before and after a distance request on the same handle (one
    staging buffer, one shared threshold word) return the bits they returned before it; after mi355rec_rebuild_replica the
    norms are taken again from the rows as they are then."""
    import torch
    from spotify_recommender_amd import CosineEngine, capi
    n = 70_001
    feats = oracle.mt19937_uniform(23, n)
    rows = [7, 7_000, 69_999]
    m = mean_sqdist(feats, feats[rows])
    want = expected_from_m(feats, m, rows + [8, 9], 200, WHERE)
    dev = torch.from_numpy(feats).to("cuda:0")                    # borrowed: the caller may overwrite it and rebuild
    with CosineEngine(dev) as eng:
        eng.set_replica(capi.REPLICA_ON)
        cos_before = eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE)
        cos_value_before = eng.query_mean_topn(feats[rows], 10)
        check(eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE), want, "parent")
        check_scores(eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE), cos_before, "cosine by row after a distance request")
        check(eng.query_nearest(feats[rows], 200, rows + [8, 9], where=WHERE), want, "parent by value")
        check_scores(eng.query_mean_topn(feats[rows], 10), cos_value_before, "cosine by value after a distance request")
        # the matrix changes under the handle: rebuild, and the norms follow (before any lane: a group's replicas are not rebuilt)
        changed = feats.copy()
        changed[:, 10] *= np.float32(3.0)
        m2 = mean_sqdist(changed, changed[rows])
        for now, m_now in ((changed, m2), (feats, m)):
            dev.copy_(torch.from_numpy(now))
            torch.cuda.synchronize()
            eng.rebuild_replica()
            check(eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE), expected_from_m(now, m_now, rows + [8, 9], 200, WHERE), "after a rebuild")
        lane = eng.lane()
        try:
            check(lane.query_nearest_rows(rows, 200, [8, 9], where=WHERE), want, "lane")
            check(eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE), want, "parent, after the lane's call")
            check_scores(lane.query_playlist_topn(rows, 300, [8, 9], where=WHERE), cos_before, "cosine on the lane")
        finally:
            lane.close()


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(10, n)
    feats[n - 5:] = feats[17]                                     # ties across the two shards
    lab = uniform_labels(n, 30, 9)
    rng = np.random.default_rng(10)
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    with NodeEngine(feats, devices=[0, 0], placement=pl) as node, CosineEngine(feats) as eng:
        fn = node._lib.mi355rec_sharded_query_distance_request
        node.set_labels(lab)
        eng.set_labels(lab)
        for k in (1, 6, 32):
            rows = [17] + [int(r) for r in rng.choice(n, size=k - 1, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            m = mean_sqdist(feats, feats[rows])
            for topn in (10, 1024):
                for kw, excluded in ((dict(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29]), rows + excl),
                                     (dict(members=feats[rows], exclude=excl), excl), (dict(rows=rows), rows)):
                    rc, ids, dist = request_call(capi, fn, node._h, topn=topn, **kw)
                    assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                    what = f"{placement} K={k} top-{topn} {sorted(kw)}"
                    check((ids, dist), _call(eng, topn=topn, **kw), what + " against the single handle")
                    check((ids, dist), expected_from_m(feats, m, excluded, topn, kw.get("where"), lab, kw.get("labels")), what)
        check(node.query_nearest_rows([3, 4], 20), eng.query_nearest_rows([3, 4], 20), "the Python methods")
        rc = request_call(capi, fn, node._h, members=feats[:2], flags=1)[0]
        assert rc == capi.ERR_INVALID_ARG and "must be 0" in node._lib.mi355rec_sharded_last_error(node._h).decode()
