"""Parity sweep of the matrix-core batch path (csrc/batched.hip.h, csrc/engine_batch.hip.h) forced onto the shards it has
never seen: 1 to 131 073 rows around every boundary the host code and the kernels branch on, batch sizes at the edges of
the NB ladder, topn at kMultiMaxTopK, hostile catalogues, shards with a row_base, duplicate queries, the served / queued
edge of the pre-filter, step 2 of pass 1, and the exact multi-query pass across its chain.  The cases, and where each number
comes from, are in tests/batched_sweep_cases.py; tests/test_batched_sweep_cpu.py runs the small ones through the CPU backend.

Every query of every batch: score bits equal to oracle.scores, ids tie-aware against oracle.topn_heap, the count and the
padding (mi355rec_query_batch_topn); the packed keys of mi355rec_enqueue_batch_keys equal to that result and to
mi355rec_enqueue_query_keys on the same handle.  No tolerance anywhere.  mi355rec_batched_last_counters keeps the sweep from
testing only the exact queue: on uniform catalogues the number of queued queries is derived, not observed."""
import numpy as np
import pytest

from oracle import oracle
from tests import batched_sweep_cases as cases
from tests.parity import assert_topn_matches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def Engine(torch_cuda):
    from spotify_recommender_amd.engine import CosineEngine
    return CosineEngine


def batch_keys(eng, torch, q, e, eff, how="host"):
    """The packed keys [batch, eff] of one asynchronous batched call."""
    batch = q.shape[0]
    keys = torch.zeros(batch * eff, dtype=torch.int64, device="cuda")
    if how == "host":
        eng.enqueue_batch_keys(q, e, eff, keys)
    elif how == "streamed":
        eng.enqueue_batch_keys_streamed(q, e, eff, keys)
        eng.enqueue_flush()
    else:
        qd, ed = torch.from_numpy(np.array(q)).cuda(), torch.from_numpy(np.array(e)).cuda()
        torch.cuda.synchronize()
        eng.enqueue_batch_keys_dev(qd, ed, eff, keys)
    torch.cuda.synchronize()
    return keys.cpu().numpy().reshape(batch, eff)


def single_keys(eng, torch, q, e, eff):
    """The same queries one at a time through mi355rec_enqueue_query_keys."""
    batch = q.shape[0]
    keys = torch.zeros((batch, eff), dtype=torch.int64, device="cuda")
    for b in range(batch):
        eng.enqueue_query_keys(q[b], int(e[b]), eff, keys[b])
    torch.cuda.synchronize()
    return keys.cpu().numpy()


def run_case(eng, torch, case, oracle_check=True, singles=True):
    """One case on a handle over its catalogue: the synchronous call against the oracle (every query), its counters, the
    asynchronous call's keys against it and against the single-query path.  Returns (keys, counters)."""
    from spotify_recommender_amd.engine import unpack_keys
    q, e, _ = case.queries()
    eng.set_batch_path(case.path)
    eng.set_replica(case.replica)
    before = eng.stats()
    idx, sc, counts = cases.batch_padded(eng, q, e, case.topn)
    after = eng.stats()
    assert after.route_mfma_two_pass - before.route_mfma_two_pass == (case.chunks if case.on_path else 0), f"{case}: not the path it is aimed at"
    d = None
    if case.on_path:
        d = eng.batched_last_counters()
        cases.check_counters(case, d)
    elif case.path == cases.BATCH_MULTI:
        assert after.route_multi_fp32 > before.route_multi_fp32, f"{case}: not the exact multi-query pass"
    for b in range(case.batch):
        c = int(counts[b])
        assert c == case.expected_count(int(e[b])), f"{case}: query {b}: count {c}"
        if oracle_check:
            cases.check_query(case, b, idx[b, :c], sc[b, :c], q, e)
    keys = batch_keys(eng, torch, q, e, case.eff)
    for b in range(case.batch):
        c = int(counts[b])
        rows, scores = unpack_keys(keys[b])
        assert not keys[b, c:].any() and len(rows) == c, f"{case}: query {b}: keys past the count"
        assert rows.tolist() == idx[b, :c].tolist(), f"{case}: query {b}: the asynchronous call's rows differ from the synchronous call's"
        assert np.array_equal((scores + np.float32(0)).view(np.uint32), (sc[b, :c] + np.float32(0)).view(np.uint32)), f"{case}: query {b}: scores"
    if singles:
        one = single_keys(eng, torch, q, e, case.eff)
        differ = np.flatnonzero((one != keys).any(axis=1))
        assert differ.size == 0, f"{case}: queries {differ[:8]} differ from the single-query path"
    return keys, d


def sweep(Engine, torch, todo):
    """Cases grouped by catalogue: one handle each, in list order."""
    handles = {}
    try:
        for case in todo:
            key = (case.n, case.kind, case.row_base)
            if key not in handles:
                handles[key] = Engine(case.feats(), row_base=case.row_base)
            run_case(handles[key], torch, case)
    finally:
        for h in handles.values():
            h.close()


@pytest.mark.parametrize("rows", list(cases.ROW_CLASSES))
def test_row_counts(Engine, torch_cuda, rows):
    sweep(Engine, torch_cuda, [c for n in cases.ROW_CLASSES[rows] for c in cases.row_cases(n)])


@pytest.mark.parametrize("batch", cases.BATCHES)
@pytest.mark.parametrize("n", cases.BATCH_ROWS)
def test_batch_sizes(Engine, torch_cuda, n, batch):
    sweep(Engine, torch_cuda, [c for c in cases.batch_cases(n) if c.batch == batch])


@pytest.mark.parametrize("n", cases.BATCH_ROWS)
def test_topn_up_to_and_past_128(Engine, torch_cuda, n):
    """run_case asserts through stats().route_mfma_two_pass that top-128 took the path and top-129 did not."""
    todo = cases.topn_cases(n)
    assert [c.on_path for c in todo] == [True, True, True, True, False]
    sweep(Engine, torch_cuda, todo)


@pytest.mark.parametrize("n", cases.HOSTILE_ROWS)
@pytest.mark.parametrize("kind", cases.HOSTILE_KINDS)
def test_hostile_kinds(Engine, torch_cuda, kind, n):
    sweep(Engine, torch_cuda, cases.hostile_cases(kind, n))


@pytest.mark.parametrize("n", cases.SOURCE_ROWS)
def test_sources_give_identical_keys(Engine, torch_cuda, n):
    """Replica-sourced (checked against the oracle), then fp32-sourced and — NB = 32 — without the tile maxima: the same keys
    and the same counters, bit for bit."""
    with Engine(cases.catalogue(n, cases.UNIFORM)) as eng:
        assert eng.stats().replica_bytes_per_query > 0, "a shard of this size has an fp16 replica"
        for case in cases.source_cases(n):
            q, e, _ = case.queries()
            keys, d = run_case(eng, torch_cuda, case)
            assert cases.expected_counters(case)["served"] > 0
            ways = [("fp32-sourced", cases.BATCH_MFMA, cases.REPLICA_OFF)]
            if cases.nb_of(case.batch) >= 16:
                pairs = eng.batched_pass2_pairs()
                assert pairs["pairs_done"] < pairs["pairs_total"], f"{case}: the kTileMax form skipped nothing: {pairs}"
                ways.append(("NOSKIP", cases.BATCH_MFMA_NOSKIP, cases.REPLICA_AUTO))
            for name, path, replica in ways:
                eng.set_batch_path(path)
                eng.set_replica(replica)
                other = batch_keys(eng, torch_cuda, q, e, case.eff)
                d2 = eng.batched_last_counters()
                assert np.array_equal(other, keys), f"{case}: {name} keys differ from the replica-sourced run"
                assert d2 == d, f"{case}: {name} counters {d2}, replica-sourced {d}"
                if name == "NOSKIP":
                    pairs = eng.batched_pass2_pairs()
                    assert pairs["pairs_done"] == pairs["pairs_total"], pairs


def test_replica_built_on_demand_below_65536_rows(Engine, torch_cuda):
    todo = cases.replica_on_demand_cases()
    with Engine(todo[0].feats()) as eng:
        assert eng.stats().replica_bytes_per_query == 0
        eng.set_replica(cases.REPLICA_ON)
        assert eng.stats().replica_bytes_per_query > 0
        for case in todo:
            keys, d = run_case(eng, torch_cuda, case)
            q, e, _ = case.queries()
            eng.set_replica(cases.REPLICA_OFF)
            other = batch_keys(eng, torch_cuda, q, e, case.eff)
            assert np.array_equal(other, keys) and eng.batched_last_counters() == d, f"{case}: fp32-sourced run differs"


@pytest.mark.parametrize("n", [65, 4097])
def test_shards_with_a_row_base(Engine, torch_cuda, n):
    sweep(Engine, torch_cuda, cases.shard_cases(n))


def test_duplicate_queries(Engine, torch_cuda):
    sweep(Engine, torch_cuda, cases.duplicate_cases())


@pytest.mark.parametrize("topn", [1, 10, 128])
def test_served_queued_edge(Engine, torch_cuda, topn):
    """Each case on a handle of its own (its first batched call): below the edge every query is queued, from it on only the
    four the bound cannot be claimed for — check_counters asserts it from the derivation in the case module."""
    for case, served in cases.edge_cases(topn):
        want = cases.expected_counters(case)
        assert (want["served"] > 0) == served and want["queued_queries"] == (4 if served else case.batch)
        sweep(Engine, torch_cuda, [case])


def test_step_two_of_pass_one(Engine, torch_cuda):
    """The smallest shard on which pass 1 looks at every second tile only (bq_step1, engine_batch.hip.h:366-371), and one
    ragged tile more: 33 queries, top-10, every list equal to the single-query path, four against the oracle.  The row
    count comes from the grid the handle reports; this is the smallest shape that reaches the branch."""
    torch = torch_cuda
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import unpack_keys
    with Engine(cases.catalogue(4097, cases.UNIFORM)) as probe:
        probe.set_batch_path(capi.BATCH_MFMA)
        q, e, _ = cases.Case("probe", 4097, cases.UNIFORM, 33, 10).queries()
        probe.query_batch_topn(q, e, 10)
        grid = probe.stats().batched_grid_blocks
    assert 0 < grid <= 1280
    n_lo, n_hi = cases.step2_rows(grid)
    assert cases.step1_of(n_lo, grid) == 2 and cases.step1_of(n_lo - 64, grid) == 1 and cases.step1_of(n_hi, grid) == 2
    feats = oracle.mt19937_uniform(cases.SEED % 100_000, n_hi)
    dev = torch.from_numpy(feats).cuda()
    rng = np.random.default_rng(cases.SEED)
    for n in (n_lo, n_hi):
        rows = rng.choice(n, size=33, replace=False)
        rows[0], rows[1] = n - 1, n - 64                       # the last row and one of the last full tile
        q = feats[rows].copy()
        e = rows.astype(np.int64)
        q[2::4] = rng.random((len(q[2::4]), 12), dtype=np.float32)
        e[2::4] = -1
        with Engine(dev[:n]) as eng:
            assert eng.stats().batched_grid_blocks in (0, grid)
            keys = torch.zeros(33 * 10, dtype=torch.int64, device="cuda")
            eng.enqueue_batch_keys(q, e, 10, keys)             # AUTO: 33 queries go to the matrix-core path
            torch.cuda.synchronize()
            assert eng.stats().route_mfma_two_pass == 1 and eng.stats().batched_grid_blocks == grid
            d = eng.batched_last_counters()
            assert d["queued_queries"] == 0 and d["candidates_total"] >= 33 and d["special_rows"] == 0, d
            got = keys.cpu().numpy().reshape(33, 10)
            assert np.array_equal(single_keys(eng, torch, q, e, 10), got), "a list differs from the single-query path"
        for b in (0, 1, 2, 32):
            want = oracle.scores(feats[:n], q[b], threads=0)
            r_, s_ = unpack_keys(got[b])
            assert_topn_matches(r_, s_, want, int(e[b]), 10, ref_idx=oracle.topn_heap(want, int(e[b]), 10))


@pytest.mark.parametrize("n", cases.CHAIN_ROWS)
def test_exact_multi_query_pass_across_its_chain(Engine, torch_cuda, n):
    sweep(Engine, torch_cuda, cases.chain_cases(n))


def test_device_resident_and_streamed_entry_points(Engine, torch_cuda):
    """mi355rec_enqueue_batch_keys_dev once per NB, and mi355rec_enqueue_batch_keys_streamed + mi355rec_enqueue_flush (with the
    path forced nothing is streamed: the batch is served at once, mi355rec.hip:426-432): the keys of mi355rec_enqueue_batch_keys."""
    todo = cases.entry_cases()
    assert sorted(cases.nb_of(c.batch) for c in todo) == [1, 2, 4, 8, 16, 32]
    with Engine(todo[0].feats()) as eng:
        for case in todo:
            q, e, _ = case.queries()
            keys, d = run_case(eng, torch_cuda, case, oracle_check=case.batch not in cases.BATCHES, singles=False)
            routed = eng.stats().route_mfma_two_pass
            dev = batch_keys(eng, torch_cuda, q, e, case.eff, how="dev")
            d2 = eng.batched_last_counters()
            assert eng.stats().route_mfma_two_pass == routed + 1 and d2["queued_queries"] == d["queued_queries"] == 4, (d, d2)
            assert np.array_equal(dev, keys), f"{case}: device-resident queries give other keys"
        case = cases.Case("streamed", 4097, cases.UNIFORM, 33, 10)
        q, e, _ = case.queries()
        keys, d = run_case(eng, torch_cuda, case, oracle_check=False, singles=False)
        streamed = batch_keys(eng, torch_cuda, q, e, case.eff, how="streamed")
        assert np.array_equal(streamed, keys) and eng.batched_last_counters()["queued_queries"] == d["queued_queries"] == 4
