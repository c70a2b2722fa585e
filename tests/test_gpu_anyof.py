"""ANY-OF REQUESTS on the MI355X (csrc/anyof.hip.h: anyof_scan_kernel, its per-member cut over the 8-bit replica, its attribution
launch), through mi355rec_query_anyof_request and its node-handle twin, bit for bit against tests/anyof_oracle.py: ids, score bits,
member indices, counts and padding, no tolerances.  Sizes at the quad, the 2048-row tile, kPlBoundRows, the 4096-row anchor table
and several workgroups; without a replica (every row takes the chains) and with one (the pre-filter); one 1 M-row catalogue on which
many workgroups publish thresholds to each other.

Which copy the scan reads: the 8-bit replica whenever the handle HAS one, so "replica off" is a handle that never built one and
"replica on" one that did (set_replica(ON) builds it on demand), as in tests/test_gpu_distance.py."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.anyof_oracle import check, expected_from_v, request_call, value
from tests.distance_oracle import hostile_catalogue
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
    rc, ids, sc, mem = request_call(capi, eng._lib.mi355rec_query_anyof_request, eng._h, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, sc, mem


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


def _member_cases(rng, feats):
    """[(k, rows, vecs, (v, a) by row, (v, a) by value)]: the oracle's values once per set of members."""
    n = feats.shape[0]
    out = []
    for k in (1, 3, 32):
        rows = [int(r) for r in rng.choice(n, size=k, replace=n < k)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = np.nan_to_num(feats[int(rng.integers(0, n))], nan=0.5, posinf=1.0, neginf=-1.0)
        out.append((k, rows, vecs, value(feats, feats[rows]), value(feats, vecs)))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    from spotify_recommender_amd import capi
    feats = oracle.mt19937_uniform(700 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    in_set = sorted({int(r) for r in rng.choice(n, size=max(1, n // 3), replace=False)})
    cases = _member_cases(rng, feats)
    results = {}
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        with eng.row_set(in_set) as rs:
            for k, rows, vecs, (v_r, a_r), (v_v, a_v) in cases:
                for topn in TOPNS:
                    what = f"n={n} [{mode}] K={k} top-{topn}"
                    got = _call(eng, rows=rows, topn=topn)
                    check(got, expected_from_v(feats, v_r, a_r, rows, topn), what + " by row")
                    results.setdefault((k, topn), []).append(got)
                    check(_call(eng, members=vecs, topn=topn), expected_from_v(feats, v_v, a_v, [], topn), what + " by value")
                    for rs_mode, only in ((capi.ROWSET_EXCLUDE, False), (capi.ROWSET_ONLY, True)):
                        check(_call(eng, members=vecs, exclude=[n - 1, 0, 0], where=WHERE, labels=WANTED, topn=topn, ext=_ext(rs, rs_mode)),
                              expected_from_v(feats, v_v, a_v, [n - 1, 0], topn, WHERE, lab, WANTED, in_set, only),
                              what + f" composed, row set mode {rs_mode}")
                # without out_member (no attribution launch, the merge notifies): the same ids and scores
                ids, sc, _ = _call(eng, rows=rows, topn=10, want_member=False)
                want = expected_from_v(feats, v_r, a_r, rows, 10)
                assert ids.tolist() == want[0].tolist() and np.array_equal(sc.view(np.uint32), want[1].view(np.uint32))
    for key, (off, on) in results.items():                        # replica on and off: identical results
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [5, 257, 4097, 70_001])
def test_hostile_rows_and_members(engine_lib, n):
    """NaN, +-inf, all-zero, 1e-30 and 1e30 rows, duplicates; members that are tiny, zero or not finite (the cut is off then)."""
    feats = hostile_catalogue(n)
    rng = np.random.default_rng([9, n])
    for mode, eng in _engines(feats):
        for k in (1, 3, 32):
            rows = [0] + [int(r) for r in rng.choice(np.arange(1, n), size=k - 1, replace=n - 1 < k - 1)]   # hostile rows among them
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            tiny = vecs.copy()
            tiny[k // 2] = np.float32(1e-30)
            zero = np.zeros((k, 12), np.float32)
            nan = vecs.copy()
            nan[k - 1, 5] = np.nan
            for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []), ("by row", dict(rows=rows), feats[rows], rows),
                                                ("tiny member", dict(members=tiny), tiny, []), ("zero members", dict(members=zero), zero, []),
                                                ("NaN member", dict(members=nan), nan, [])):
                v, a = value(feats, members)
                n_adm = n - len(set(excluded))
                for topn in sorted({1, 10, 257, 1024, max(1, min(1024, n_adm)), min(1024, n_adm + 1)}):
                    got = _call(eng, topn=topn, **kw)
                    check(got, expected_from_v(feats, v, a, excluded, topn), f"hostile n={n} [{mode}] K={k} {what} top-{topn}")
                    assert got[0].size == min(topn, n_adm)


@pytest.fixture(scope="module")
def big(engine_lib):
    """(feats, member rows, (v, a) of every row): computed once, never modified."""
    feats = oracle.mt19937_uniform(2026, N_BIG)
    rows = [123_457, 700_001, 42]
    return feats, rows, value(feats, feats[rows])


def _merged_one_member(eng, feats, rows, excluded, topn):
    """What a caller must do today: K one-member playlist requests with the whole exclusion list, the max per row, the first N."""
    best = {}
    for r in rows:
        ids, sc = eng.query_mean_topn(feats[[r]], topn, exclude=excluded)
        for i, s in zip(ids.tolist(), sc.tolist()):
            if i not in best or s > best[i]:
                best[i] = s
    order = sorted(best, key=lambda i: (-best[i], i))[:topn]
    return np.asarray(order, np.int64), np.asarray([best[i] for i in order], np.float32)


def test_1m_rows_many_workgroups_and_the_prefilter_works(big):
    """Top-10 of 1 M uniform rows, K = 3: the oracle's answer and the merged one-member requests', and rows_exact: at most n / 4 with
    the replica (the model gives well under 1 % at the true threshold; the anchors' start is looser), every row without it."""
    feats, rows, (v, a) = big
    for mode, eng in _engines(feats):
        before = eng.playlist_counters()
        got = _call(eng, rows=rows, topn=10)
        after = eng.playlist_counters()
        exact = after["rows_exact"] - before["rows_exact"]
        print(f"[{mode}] rows_exact {exact} of {N_BIG} ({100.0 * exact / N_BIG:.3f} %)")
        check(got, expected_from_v(feats, v, a, rows, 10), f"1 M rows [{mode}]")
        assert after["queries"] - before["queries"] == 1
        if mode == "replica on":
            assert 0 < exact <= N_BIG // 4, exact
            ui, us = _merged_one_member(eng, feats, rows, rows, 10)
            assert got[0].tolist() == ui.tolist() and np.array_equal(got[1].view(np.uint32), us.view(np.uint32))
            got = _call(eng, rows=rows, exclude=[5, 6], where=WHERE, topn=100)          # the other shapes on many workgroups
            check(got, expected_from_v(feats, v, a, rows + [5, 6], 100, WHERE), "1 M rows, by row, composed")
        else:
            assert exact == N_BIG, exact


def test_lanes_updates_and_interleaving(engine_lib):
    """A lane gives its parent's bits; playlist and distance requests before and after an any-of request on the same handle (one
    staging buffer, one shared threshold word) return the bits they returned before it; after update_rows on 1 % of the rows the
    call equals a fresh handle's."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    n = 70_001
    feats = oracle.mt19937_uniform(23, n)
    rows = [7, 7_000, 69_999]
    v, a = value(feats, feats[rows])
    want = expected_from_v(feats, v, a, rows + [8, 9], 200, WHERE)
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        cos_before = eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE)
        dist_before = eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE)
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent")
        check(engine.query_anyof(eng, 200, rows=rows, exclude=[8, 9], where=WHERE), want, "the Python function")
        check_scores(eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE), cos_before, "cosine by row after an any-of request")
        check_scores(eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE), dist_before, "distance after an any-of request")
        lane = eng.lane()
        try:
            check(_call(lane, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "lane")
            check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent, after the lane's call")
            check_scores(lane.query_playlist_topn(rows, 300, [8, 9], where=WHERE), cos_before, "cosine on the lane")
        finally:
            lane.close()
        # 1 % of the rows change in place (some of them towards a member): the call answers as a fresh handle does
        rng = np.random.default_rng(70)
        changed_rows = np.sort(rng.choice(n, size=n // 100, replace=False))
        changed = feats.copy()
        changed[changed_rows] = rng.random((changed_rows.size, 12), dtype=np.float32)
        changed[changed_rows[:20]] = feats[7] * np.float32(1.5)
        eng.update_rows(changed_rows, changed[changed_rows])
        v2, a2 = value(changed, changed[rows])
        want2 = expected_from_v(changed, v2, a2, rows + [8, 9], 200, WHERE)
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "after update_rows")
    with CosineEngine(changed) as fresh:
        fresh.set_replica(capi.REPLICA_ON)
        check(_call(fresh, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "a fresh handle")


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(10, n)
    feats[n - 5:] = feats[17]                                     # ties across the two shards
    lab = uniform_labels(n, 30, 9)
    rng = np.random.default_rng(10)
    seen = sorted({int(r) for r in rng.choice(n, size=n // 4, replace=False)})
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    with NodeEngine(feats, devices=[0, 0], placement=pl) as node, CosineEngine(feats) as eng:
        fn = node._lib.mi355rec_sharded_query_anyof_request
        node.set_labels(lab)
        eng.set_labels(lab)
        for k in (1, 6, 32):
            rows = [17] + [int(r) for r in rng.choice(n, size=k - 1, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            v, a = value(feats, feats[rows])
            for topn in (10, 1024):
                for kw, excluded in ((dict(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29]), rows + excl),
                                     (dict(members=feats[rows], exclude=excl), excl), (dict(rows=rows), rows)):
                    rc, ids, sc, mem = request_call(capi, fn, node._h, topn=topn, **kw)
                    assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                    what = f"{placement} K={k} top-{topn} {sorted(kw)}"
                    check((ids, sc, mem), _call(eng, topn=topn, **kw), what + " against the single handle")
                    check((ids, sc, mem), expected_from_v(feats, v, a, excluded, topn, kw.get("where"), lab, kw.get("labels")), what)
        v, a = value(feats, feats[[3, 4]])
        for kw, rs in ((dict(seen=seen), dict(rowset=seen, rowset_only=False)), (dict(only=seen), dict(rowset=seen, rowset_only=True))):
            got = engine.query_anyof(node, 20, rows=[3, 4], **kw)
            check(got, engine.query_anyof(eng, 20, rows=[3, 4], **kw), "the Python function, node against single handle")
            check(got, expected_from_v(feats, v, a, [3, 4], 20, **rs), "the Python function with a row set")
        rc = request_call(capi, fn, node._h, members=feats[:2], flags=1)[0]
        assert rc == capi.ERR_INVALID_ARG and "must be 0" in node._lib.mi355rec_sharded_last_error(node._h).decode()
