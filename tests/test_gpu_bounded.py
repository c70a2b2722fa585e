"""BOUNDED REQUESTS on the MI355X (csrc/playlist.hip.h, "BOUNDED": the count launch of playlist_scan_kernel, topk == 0 without a
candidate list; csrc/engine_playlist.hip.h: the count launch, the seeded top-N launch and the host's cut at the floor), through
mi355rec_query_bounded_request and its node-handle twin, against tests/bounded_oracle.py: ids, value bits, totals, counts and
padding, no tolerances.  Sizes at the quad (4 rows), the 2048-row tile and several workgroups (tiles are dealt round-robin); without
a replica (every row takes the chains) and with one (the pre-filter at its final cut from the first tile).

Which copy the scan reads: the 8-bit replica whenever the handle HAS one, so "replica off" is a handle that never built one and
"replica on" one that did (set_replica(ON) builds it on demand), as in tests/test_gpu_distance.py."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import bounded_oracle as bo
from tests.distance_oracle import hostile_catalogue
from tests.playlist_labels_oracle import uniform_labels

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 3, 4, 5, 2047, 2048, 2049, 4097, 65_537]
METRICS = ((bo.COSINE, "cosine"), (bo.EUCLIDEAN, "euclidean"))


def _call(eng, **kw):
    from spotify_recommender_amd import capi
    rc, ids, sc, total = bo.request_call(capi, eng._lib.mi355rec_query_bounded_request, eng._h, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, sc, total


def _ext(rowset, mode):
    from spotify_recommender_amd import capi
    return capi.RequestExt(ctypes.sizeof(capi.RequestExt), mode, None, rowset._ptr())


def _engines(feats):
    """("replica off", engine) then ("replica on", engine), one alive at a time."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    """K = 1, 2, 32 by row and by value, both metrics; floors at -1, above 1, exactly a row's value and one step past it (the 10th,
    1 000th and median row); topn 0, below, equal to and above the total; composed with an exclusion list that holds matching rows
    and duplicates, a filter, a label set and a row set of either mode.  Replica on and off: identical."""
    from spotify_recommender_amd import capi
    feats = oracle.mt19937_uniform(900 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    in_set = sorted({int(r) for r in rng.choice(n, size=max(1, n // 3), replace=False)})
    cases = []
    for k in (1, 2, 32):
        rows = [int(r) for r in rng.choice(n, size=k, replace=n < k)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = feats[int(rng.integers(0, n))]
        for metric, _ in METRICS:
            for kw, members, excluded in ((dict(rows=rows), feats[rows], rows), (dict(members=vecs), vecs, [])):
                v = bo.values(feats, members, metric)
                ok = bo.admissible(feats, v, excluded)
                best = np.flatnonzero(ok)[np.argsort(-bo.image(v[ok]).astype(np.int64), kind="stable")[:3]].tolist() if ok.any() else []
                excl = best + best[:1] + [n - 1, 0]               # matching rows, a duplicate id, the tail row
                composed = [(excl, None, None, None, False), ([], WHERE, None, None, False), ([], None, WANTED, None, False),
                            ([], None, None, in_set, False), (excl, WHERE, WANTED, in_set, True)]
                # the oracle's answers, once for both handles: [(what, call arguments, row-set mode or None, expected)]
                bounds = bo.bounds_for(v, ok, metric)
                for bound in bounds:
                    what = f"n={n} K={k} metric={metric} {sorted(kw)} bound={bound!r}"
                    total = bo.expected_from_values(v, ok, metric, bound, 0)[2]
                    for topn in bo.topns_for(total):
                        cases.append((what + f" top-{topn}", dict(kw, metric=metric, bound=bound, topn=topn), None,
                                      bo.expected_from_values(v, ok, metric, bound, topn)))
                    if bound not in (bounds[0], bounds[-2], bounds[-1]):
                        continue                                  # composed: at everything, and at the median row and one step past it
                    for ex, where, wanted, rowset, only in composed:
                        ok_c = bo.admissible(feats, v, excluded + ex, where, lab, wanted, rowset, only)
                        mode = None if rowset is None else capi.ROWSET_ONLY if only else capi.ROWSET_EXCLUDE
                        cases.append((what + f" composed {bool(ex), where, wanted, mode}",
                                      dict(kw, metric=metric, bound=bound, topn=10, exclude=ex, where=where, labels=wanted), mode,
                                      bo.expected_from_values(v, ok_c, metric, bound, 10)))
    results = []
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        with eng.row_set(in_set) as rs:
            got_all = []
            for what, kw, rs_mode, want in cases:
                got = _call(eng, ext=_ext(rs, rs_mode) if rs_mode is not None else None, **kw)
                bo.check(got, want, f"[{mode}] {what}")
                got_all.append(got)
            results.append(got_all)
            kw = dict(cases[0][1], topn=10)
            assert _call(eng, want_score=False, **kw)[0].tolist() == _call(eng, **kw)[0].tolist()   # out_score is optional
    for (what, _, _, _), off, on in zip(cases, *results):       # replica on and off: identical results
        bo.check(on, off, f"{what}: replica on against off")


@pytest.mark.parametrize("n", [5, 257, 4097])
def test_hostile_rows(engine_lib, n):
    """NaN, +-inf, all-zero, 1e-30 and 1e30 rows (the replica's special rows) and duplicates: radius 0 counts the duplicates, a
    row whose m is not finite never matches, a zero row scores +0.0 and matches a floor of either zero."""
    feats = hostile_catalogue(n)
    rng = np.random.default_rng([9, n])
    for mode, eng in _engines(feats):
        for k in (1, 2, 32):
            rows = [0] + [int(r) for r in rng.choice(np.arange(1, n), size=k - 1, replace=n - 1 < k - 1)]
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            for metric, _ in METRICS:
                for kw, members, excluded in ((dict(members=vecs), vecs, []), (dict(rows=rows), feats[rows], rows)):
                    v = bo.values(feats, members, metric)
                    ok = bo.admissible(feats, v, excluded)
                    for bound in bo.bounds_for(v, ok, metric) + [0.0, -0.0][:2 if metric == bo.COSINE else 0]:
                        for topn in (0, 10, 1024):
                            bo.check(_call(eng, metric=metric, bound=bound, topn=topn, **kw), bo.expected_from_values(v, ok, metric, bound, topn),
                                     f"hostile n={n} [{mode}] K={k} metric={metric} {sorted(kw)} bound={bound!r} top-{topn}")
        dups = [i for i in range(n) if np.array_equal(feats[i], feats[0])]
        ids, dist, total = _call(eng, metric=bo.EUCLIDEAN, members=feats[:1], bound=0.0, topn=100)
        assert ids.tolist() == dups and total == len(dups) and not dist.view(np.uint32).any()


def test_zero_floor_of_either_sign(engine_lib):
    n = 4097
    feats = np.random.default_rng(3).random((n, 12), dtype=np.float32) - np.float32(0.5)
    feats[[5, 77, 2048, 4096]] = 0.0
    v = bo.values(feats, feats[[1, 2]], bo.COSINE)
    ok = bo.admissible(feats, v, [1, 2])
    for mode, eng in _engines(feats):
        plus = _call(eng, rows=[1, 2], bound=0.0, topn=1024)
        bo.check(plus, bo.expected_from_values(v, ok, bo.COSINE, 0.0, 1024), f"+0.0 [{mode}]")
        bo.check(_call(eng, rows=[1, 2], bound=-0.0, topn=1024), plus, f"-0.0 against +0.0 [{mode}]")
        assert _call(eng, rows=[1, 2], bound=0.0, topn=0)[2] == plus[2] >= 4


def test_independent_of_the_oracle_at_4097_rows(engine_lib):
    """total = the number of candidate_scores values >= bound over every row; the results = the unbounded request's, filtered."""
    from spotify_recommender_amd import engine
    n = 4097
    feats = oracle.mt19937_uniform(77, n)
    rows = [11, 2050, 4096]
    for mode, eng in _engines(feats):
        values, adm = engine.candidate_scores(eng, np.arange(n), rows=rows, exclude=[5, 6])
        top_ids, top_sc = eng.query_playlist_topn(rows, 1024, [5, 6])
        for bound in (float(np.sort(values[adm])[-10]), float(np.median(values[adm])), 0.99999, -1.0):
            ids, sc, total = engine.query_bounded(eng, 1024, bound, rows=rows, exclude=[5, 6])
            assert total == int(np.count_nonzero(values[adm] >= np.float32(bound))), (mode, bound)
            keep = top_sc >= np.float32(bound)
            assert ids.tolist() == top_ids[keep].tolist() and np.array_equal(sc.view(np.uint32), top_sc[keep].view(np.uint32)), (mode, bound)
        dist_v, dist_adm = engine.candidate_scores(eng, np.arange(n), rows=rows, metric="distance")
        near_ids, near_d = eng.query_nearest_rows(rows, 1024)
        for radius in (float(near_d[9]), float(np.nextafter(near_d[9], np.float32(0))), float(np.median(dist_v[dist_adm]))):
            ids, d, total = engine.query_bounded(eng, 1024, radius, metric="euclidean", rows=rows)
            assert total == int(np.count_nonzero(dist_v[dist_adm] <= np.float32(radius))), (mode, radius)
            keep = near_d <= np.float32(radius)
            assert ids.tolist() == near_ids[keep].tolist() and np.array_equal(d.view(np.uint32), near_d[keep].view(np.uint32)), (mode, radius)


def test_lanes_updates_counters_and_interleaving(engine_lib):
    """A lane gives its parent's bits; a playlist and a distance request around a bounded one on the same handle (one staging buffer,
    one shared threshold word) return the bits they returned before; after update_rows with rows moved across the floor the call
    equals the oracle on the updated matrix; mi355rec_playlist_counters counts a bounded call once, and rows_exact does not move for a
    count-only call."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    n = 70_001
    feats = oracle.mt19937_uniform(24, n)
    rows = [7, 7_000, 69_999]
    v = bo.values(feats, feats[rows], bo.COSINE)
    ok = bo.admissible(feats, v, rows + [8, 9], WHERE)
    bound = float(np.sort(v[ok])[-500])
    want = bo.expected_from_values(v, ok, bo.COSINE, bound, 200)
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        cos_before = eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE)
        dist_before = eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE)
        before = eng.playlist_counters()
        bo.check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, bound=bound, topn=200), want, "parent")
        mid = eng.playlist_counters()
        assert mid["queries"] - before["queries"] == 1
        assert _call(eng, rows=rows, exclude=[8, 9], where=WHERE, bound=bound, topn=0)[2] == want[2] == 500
        after = eng.playlist_counters()
        assert after["queries"] - mid["queries"] == 1 and after["rows_exact"] == mid["rows_exact"], "a count launch moves rows_exact"
        bo.check(engine.query_bounded(eng, 200, bound, rows=rows, exclude=[8, 9], where=WHERE), want, "the Python function")
        for a, b in zip(eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE), cos_before):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
        for a, b in zip(eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE), dist_before):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
        lane = eng.lane()
        try:
            bo.check(_call(lane, rows=rows, exclude=[8, 9], where=WHERE, bound=bound, topn=200), want, "lane")
            bo.check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, bound=bound, topn=200), want, "parent, after the lane's call")
        finally:
            lane.close()
        # rows move across the floor: matching rows become random ones, random rows become near copies of a member
        rng = np.random.default_rng(71)
        changed = feats.copy()
        down = want[0][:40]
        up = np.setdiff1d(rng.choice(n, size=60, replace=False), np.concatenate([want[0], rows, [8, 9]]))
        changed[down] = rng.random((down.size, 12), dtype=np.float32)
        changed[up] = feats[7] * np.float32(1.01)
        moved = np.sort(np.concatenate([down, up]))
        eng.update_rows(moved, changed[moved])
        v2 = bo.values(changed, changed[rows], bo.COSINE)
        ok2 = bo.admissible(changed, v2, rows + [8, 9], WHERE)
        want2 = bo.expected_from_values(v2, ok2, bo.COSINE, bound, 200)
        assert want2[2] != want[2] or want2[0].tolist() != want[0].tolist()
        bo.check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, bound=bound, topn=200), want2, "after update_rows")


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(11, n)
    feats[n - 5:] = feats[17]                                     # ties across the two shards
    lab = uniform_labels(n, 30, 9)
    rng = np.random.default_rng(10)
    seen = sorted({int(r) for r in rng.choice(n, size=n // 4, replace=False)})
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    with NodeEngine(feats, devices=[0, 0], placement=pl) as node, CosineEngine(feats) as eng:
        fn = node._lib.mi355rec_sharded_query_bounded_request
        node.set_labels(lab)
        eng.set_labels(lab)
        for k in (1, 32):
            rows = [17] + [int(r) for r in rng.choice(n, size=k - 1, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            for metric, name in METRICS:
                v = bo.values(feats, feats[rows], metric)
                for kw, excluded in ((dict(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29]), rows + excl),
                                     (dict(members=feats[rows], exclude=excl), excl), (dict(rows=rows), rows)):
                    ok = bo.admissible(feats, v, excluded, kw.get("where"), lab, kw.get("labels"))
                    for bound in bo.bounds_for(v, ok, metric)[:4]:
                        for topn in (0, 10, 1024):
                            rc, ids, sc, total = bo.request_call(capi, fn, node._h, metric=metric, bound=bound, topn=topn, **kw)
                            assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                            what = f"{placement} K={k} {name} bound={bound!r} top-{topn} {sorted(kw)}"
                            bo.check((ids, sc, total), _call(eng, metric=metric, bound=bound, topn=topn, **kw), what + " against the single handle")
                            bo.check((ids, sc, total), bo.expected_from_values(v, ok, metric, bound, topn), what)
        v = bo.values(feats, feats[[3, 4]], bo.COSINE)
        bound = float(np.sort(v)[n - 2_000])
        for kw, only in ((dict(seen=seen), False), (dict(only=seen), True)):
            got = engine.query_bounded(node, 20, bound, rows=[3, 4], **kw)
            bo.check(got, engine.query_bounded(eng, 20, bound, rows=[3, 4], **kw), "the Python function, node against single handle")
            bo.check(got, bo.expected_from_values(v, bo.admissible(feats, v, [3, 4], rowset=seen, rowset_only=only), bo.COSINE, bound, 20), "with a row set")
        rc = bo.request_call(capi, fn, node._h, members=feats[:2], flags=1)[0]
        assert rc == capi.ERR_INVALID_ARG and "must be 0" in node._lib.mi355rec_sharded_last_error(node._h).decode()


def test_one_shard_forwards(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 9_001
    feats = hostile_catalogue(n)
    rows = [0, 100, 9_000]
    for metric, name in METRICS:
        v = bo.values(feats, feats[rows], metric)
        ok = bo.admissible(feats, v, rows + [1], WHERE)
        bound = bo.bounds_for(v, ok, metric)[-2]
        with NodeEngine(feats, devices=[0], placement=capi.PLACEMENT_AUTO) as node:
            bo.check(engine.query_bounded(node, 50, bound, metric=name, rows=rows, exclude=[1], where=WHERE),
                     bo.expected_from_values(v, ok, metric, bound, 50), f"one shard, {name}")
