"""ROW UPDATES on the GPU (include/mi355rec_diag.h; csrc/engine_update.hip.h, the update job of q8_build_kernel): after
mi355rec_update_rows every route answers as a handle freshly created from the updated matrix would.  Expectations are the
existing oracles on the updated numpy matrix (tests/update_rows_cases.py: ids and score bits equal, no tolerance).

Sizes: 1, 4, 5, 7, 8, 9 (the tails of the fp16 pairs and the 8-bit quads, which an update must never write past), 257, 2049,
4097 (tile and anchor-table edges), 65 537 (the staging chunk of 65 536 rows, by updating every row in one call) — each on a
handle without replicas and on one with them, one handle alive at a time.

The stale bucketed sample: 655 360 rows would make 64 regions by arithmetic, but a handle builds the structure only where the
8-bit scan takes exact sample values, from 2 097 153 rows on an MI355X (tests/test_gpu_bucket_sample.py, N_MIN and
test_no_structure_below_the_exact_sample).  The stale-sample case therefore runs at 2 097 153 rows, the smallest size at which
it can; 655 360 rows assert that no structure exists and run the same update without it."""
import ctypes

import numpy as np
import pytest

from tests.update_rows_cases import adversarial_steps, catalogue, check_routes, check_single, new_rows, update_lists
from tests.playlist_labels_oracle import uniform_labels

pytestmark = pytest.mark.gpu

SIZES = [1, 4, 5, 7, 8, 9, 257, 2049, 4097, 65537]
N_BUCKET = 2_097_153


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def capi():
    from spotify_recommender_amd import capi
    return capi


@pytest.fixture(scope="module")
def Engine(torch_cuda):
    from spotify_recommender_amd.engine import CosineEngine
    return CosineEngine


def streamed_by_row(eng, torch):
    """(rows, topn) -> [(ids, scores)]: a stream of queries by row on the handle's own stream, then the flush."""
    from spotify_recommender_amd.engine import unpack_keys

    def run(rows, topn):
        outs = [torch.zeros(topn, dtype=torch.int64, device="cuda:0") for _ in rows]
        torch.cuda.synchronize()
        s = eng.own_stream()
        for r, o in zip(rows, outs):
            eng.enqueue_row_keys_streamed(int(r), topn, o, stream=s)
        eng.enqueue_flush(stream=s)
        torch.cuda.synchronize()
        return [unpack_keys(o.cpu().numpy()) for o in outs]
    return run


def make(Engine, capi, feats, replica):
    eng = Engine(feats, flags=0 if replica else capi.CREATE_NO_REPLICA)
    if replica:
        eng.set_replica(capi.REPLICA_ON)
    return eng


def side_data(n):
    rng = np.random.default_rng(n)
    return uniform_labels(n, 6, n), rng.random(n, dtype=np.float32)


@pytest.mark.parametrize("replica", [False, True], ids=["fp32", "replica"])
@pytest.mark.parametrize("n", SIZES)
def test_update_lists(Engine, capi, torch_cuda, n, replica):
    cur = catalogue(n)
    rng = np.random.default_rng(n + 1)
    labels, priors = side_data(n)
    q = n // 3
    with make(Engine, capi, cur, replica) as eng:
        eng.set_labels(labels)
        eng.set_priors(priors)
        run = streamed_by_row(eng, torch_cuda)
        eng.query_nearest_rows([q], 1)   # (a handle with replicas builds its norms here: the updates below keep them exact)
        for name, rows in update_lists(n, rng).items():
            new = new_rows(cur, rows, q, rng)
            cur[rows] = new
            eng.update_rows(rows, new)
            check_routes(eng, cur, q, f"n={n} {name}", labels, priors, run)
        info = eng.update_info()
        assert info["calls"] == len(update_lists(n, rng)) and info["rows"] == info["rows_since_snapshot"] > 0, info
        eng.update_rows([], np.empty((0, 12), np.float32))     # count == 0: succeeds, changes nothing
        assert eng.update_info()["calls"] == info["calls"]


@pytest.mark.parametrize("replica", [False, True], ids=["fp32", "replica"])
@pytest.mark.parametrize("n", SIZES)
def test_hostile_contents(Engine, capi, torch_cuda, n, replica):
    cur = catalogue(n)
    rng = np.random.default_rng(n + 2)
    labels, priors = side_data(n)
    q = n // 3
    topn = 1 if n < 16 else 10
    with make(Engine, capi, cur, replica) as eng:
        eng.set_labels(labels)
        eng.set_priors(priors)
        run = streamed_by_row(eng, torch_cuda)
        eng.query_nearest_rows([q], 1)
        for name, rows, new in adversarial_steps(cur, q, topn, rng):
            cur[rows] = new
            eng.update_rows(rows, new)
            check_single(eng.query_row_topn(q, topn), cur, cur[q], q, topn, f"n={n} {name}")
            check_routes(eng, cur, q, f"n={n} {name}", labels, priors, run, batches=(2, 33))


@pytest.mark.parametrize("n", [5, 4097, 65537])
def test_replica_entries_equal_a_fresh_handle(Engine, capi, n):
    cur = catalogue(n)
    rng = np.random.default_rng(n + 3)
    all_rows = np.arange(n)
    with make(Engine, capi, cur, True) as eng:
        eng.query_nearest_rows([0], 1)                     # norms built
        for name, rows in update_lists(n, rng).items():
            new = rng.random((len(rows), 12), dtype=np.float32)
            if name == "a tenth":                            # the special encodings among them
                new[0] = 0.0
                new[-1] = np.nan
                new[len(rows) // 2] = 1e20
            cur[rows] = new
            eng.update_rows(rows, new)
        got = eng.replica_entries(all_rows)
        scattered = eng.replica_entries(all_rows[::-3])     # (any order: one copy per run of consecutive rows)
    with make(Engine, capi, cur, True) as fresh:
        fresh.query_nearest_rows([0], 1)
        want = fresh.replica_entries(all_rows)
    for g, w, s, what in zip(got, want, scattered, ("fp16 replica", "8-bit replica", "norms")):
        assert g.tobytes() == w.tobytes(), f"n={n}: the {what} differs from a freshly created handle's"
        assert s.tobytes() == w[::-3].tobytes(), f"n={n}: {what} in scattered order"
    assert not np.isnan(got[2][1])                          # (the norms were really built and copied)


def test_replica_entries_need_replicas(Engine, capi):
    cur = catalogue(257)
    with make(Engine, capi, cur, False) as eng:
        with pytest.raises(capi.Mi355Error) as e:
            eng.replica_entries([0])
        assert e.value.code == capi.ERR_INVALID_ARG


def test_refresh_mode_over_a_borrowed_tensor(Engine, capi, torch_cuda):
    """mi355rec_create_device: the caller changes rows of its tensor, then calls with NULL."""
    torch = torch_cuda
    n = 4097
    cur = catalogue(n)
    rng = np.random.default_rng(n + 4)
    labels, priors = side_data(n)
    q = n // 3
    dev = torch.from_numpy(cur.copy()).to("cuda:0")
    with Engine(dev) as eng:
        eng.set_replica(capi.REPLICA_ON)
        eng.set_labels(labels)
        eng.set_priors(priors)
        run = streamed_by_row(eng, torch)
        eng.query_nearest_rows([q], 1)
        for name, rows in update_lists(n, rng).items():
            new = new_rows(cur, rows, q, rng)
            cur[rows] = new
            dev[torch.as_tensor(rows, device="cuda:0")] = torch.from_numpy(new).to("cuda:0")
            eng.update_rows(rows)                              # (synchronises the tensor's device, then NULL rows)
            check_routes(eng, cur, q, f"refresh {name}", labels, priors, run)
        for name, rows, new in adversarial_steps(cur, q, 10, rng):
            cur[rows] = new
            eng.update_rows(rows, new)                         # (the wrapper writes the tensor itself)
            check_routes(eng, cur, q, f"refresh {name}", labels, priors, run, batches=(12,))
        # host rows on a borrowed matrix: INVALID_ARG from the C-ABI, nothing changed
        rows = np.asarray([1, 2], np.int64)
        new = rng.random((2, 12), dtype=np.float32)
        rc = eng._lib.mi355rec_update_rows(eng._h, rows.ctypes.data_as(ctypes.c_void_p), 2, new.ctypes.data_as(ctypes.c_void_p))
        assert rc == capi.ERR_INVALID_ARG
        check_routes(eng, cur, q, "after the refused call", labels, priors, run, batches=(2,))


def test_lanes_share_an_update(Engine, capi, torch_cuda):
    torch = torch_cuda
    n = 65537
    cur = catalogue(n)
    rng = np.random.default_rng(n + 5)
    q = n // 3
    with Engine(cur) as eng:
        eng.set_replica(capi.REPLICA_ON)
        lane = eng.lane()
        try:
            runs = {"parent": streamed_by_row(eng, torch), "lane": streamed_by_row(lane, torch)}
            for h in (eng, lane):
                h.query_nearest_rows([q], 1)                   # each builds its own norms
            for through, other, name in ((eng, lane, "lane"), (lane, eng, "parent")):
                rows = sorted(int(r) for r in rng.choice(n, size=700, replace=False))
                new = rng.random((len(rows), 12), dtype=np.float32)
                cur[rows] = new
                through.update_rows(rows, new)
                check_routes(other, cur, q, f"seen by the {name}", streamed=runs[name], batches=(33,))
                for step, srows, snew in adversarial_steps(cur, q, 10, rng):
                    cur[srows] = snew
                    through.update_rows(srows, snew)
                    check_single(other.query_row_topn(q, 10), cur, cur[q], q, 10, f"{step}, seen by the {name}")
                check_routes(other, cur, q, f"hostile rows seen by the {name}", streamed=runs[name], batches=(2,))
            # a streamed query open on the lane: refused, and nothing has changed
            out = torch.zeros(10, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            s = lane.own_stream()
            lane.enqueue_row_keys_streamed(q, 10, out, stream=s)
            rows, new = [q, q + 1], rng.random((2, 12), dtype=np.float32)
            before = eng.update_info()
            with pytest.raises(capi.Mi355Error) as e:
                eng.update_rows(rows, new)
            assert e.value.code == capi.ERR_INVALID_ARG
            assert eng.update_info() == before
            lane.enqueue_flush(stream=s)
            torch.cuda.synchronize()
            check_routes(eng, cur, q, "after the refused call", streamed=runs["parent"], batches=(2,))
            cur[rows] = new
            eng.update_rows(rows, new)                         # after the lane's flush it succeeds
            check_routes(lane, cur, q, "after the flush", streamed=runs["lane"], batches=(2,))
            assert lane.update_info()["rows_since_snapshot"] == eng.update_info()["rows_since_snapshot"]
        finally:
            lane.close()


def test_a_refused_update_leaves_a_borrowed_tensor_unwritten(Engine, capi, torch_cuda):
    """Over a torch tensor the wrapper writes the rows itself: it asks the library first, so the refusal for a lane with a streamed
    query open arrives before the tensor has changed."""
    torch = torch_cuda
    n = 65537
    cur = catalogue(n)
    rng = np.random.default_rng(n + 9)
    q = n // 3
    dev = torch.from_numpy(cur.copy()).to("cuda:0")
    with Engine(dev) as eng:
        eng.set_replica(capi.REPLICA_ON)
        lane = eng.lane()
        try:
            out = torch.zeros(10, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            s = lane.own_stream()
            lane.enqueue_row_keys_streamed(q, 10, out, stream=s)
            rows, new = [q + 1, 0], rng.random((2, 12), dtype=np.float32)
            for bad in (rows, [3, 3], [n]):
                with pytest.raises(capi.Mi355Error) as e:
                    eng.update_rows(bad, rng.random((len(bad), 12), dtype=np.float32))
                assert e.value.code == capi.ERR_INVALID_ARG
            assert np.array_equal(dev.cpu().numpy().view(np.uint32), cur.view(np.uint32)), "a refused update wrote the tensor"
            lane.enqueue_flush(stream=s)
            torch.cuda.synchronize()
            check_routes(eng, cur, q, "after the refused calls", streamed=streamed_by_row(eng, torch), batches=(2,))
            cur[rows] = new
            eng.update_rows(rows, new)
            check_routes(lane, cur, q, "after the flush", streamed=streamed_by_row(lane, torch), batches=(2,))
        finally:
            lane.close()


def _stale_sample_run(Engine, capi, torch, n, want_bucketed):
    cur = np.random.default_rng(n).random((n, 12), dtype=np.float32)
    rng = np.random.default_rng(n + 6)
    q = n // 3
    with Engine(cur) as eng:
        eng.set_replica(capi.REPLICA_ON)
        has = eng.bucket_sample_info()["base_rows"] > 0
        assert has == want_bucketed, eng.bucket_sample_info()
        if want_bucketed:
            eng.set_sample(capi.SAMPLE_BUCKETED)
        rows = sorted(int(r) for r in rng.choice(n, size=n // 100, replace=False) if r != q)
        new = rng.random((len(rows), 12), dtype=np.float32)
        cur[rows] = new
        eng.update_rows(rows, new)
        for step, srows, snew in list(adversarial_steps(cur, q, 10, rng))[:2]:   # the adversarial pair
            cur[srows] = snew
            eng.update_rows(srows, snew)
        qrows = [q] + [int(r) for r in rng.choice(n, size=7, replace=False)]
        for r, got in zip(qrows, streamed_by_row(eng, torch)(qrows, 10)):
            check_single(got, cur, cur[r], r, 10, f"n={n}: streamed query of row {r} over a stale sample")
        if want_bucketed:
            assert eng.bucket_sample_info()["last_used"] == capi.SAMPLE_BUCKETED
        assert eng.update_info()["rows_since_snapshot"] == len(rows) + 2
        eng.rebuild_replica()
        assert eng.update_info()["rows_since_snapshot"] == 0


def test_a_stale_bucketed_sample_stays_exact(Engine, capi, torch_cuda):
    _stale_sample_run(Engine, capi, torch_cuda, N_BUCKET, True)


def test_64_regions_of_rows_have_no_structure_and_stay_exact(Engine, capi, torch_cuda):
    _stale_sample_run(Engine, capi, torch_cuda, 655_360, False)


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handle(capi, torch_cuda, placement):
    from spotify_recommender_amd.engine import CosineEngine, NodeEngine
    n = 4097
    cur = catalogue(n)
    rng = np.random.default_rng(n + 7)
    labels, priors = side_data(n)
    q = n // 3
    edge = (n + 1) // 2                                          # shard 0 holds rows [0, edge) of a two-shard placement
    with NodeEngine(cur, devices=[0, 0], placement=getattr(capi, "PLACEMENT_" + placement.upper())) as nd:
        nd.set_labels(labels)
        nd.set_priors(priors)
        lists = {"across the shard edge": [edge - 2, edge - 1, edge, edge + 1], "both ends": [n - 1, 0],
                 "a tenth": sorted(int(r) for r in rng.choice(n, size=n // 10, replace=False)), "all": [int(r) for r in rng.permutation(n)]}
        for name, rows in lists.items():
            new = new_rows(cur, rows, q, rng)
            old = cur.copy()
            cur[rows] = new
            tickets = [(r, nd.enqueue_row(r, 10)) for r in (q, rows[0], q + 1)]   # an open window: closed by the update ...
            nd.update_rows(rows, new)
            for r, t in tickets:                               # ... and answered from the OLD rows, whole: no scan saw a written row
                check_single(nd.wait(t, 10), old, old[r], r, 10, f"{placement} {name}: the ticket of row {r} from before the update")
            check_routes(nd, cur, q, f"{placement} {name}", labels, priors)
            with CosineEngine(cur) as single:                  # ... and equal to a single handle's answers
                for topn in (1, 10):
                    a, b = nd.query_row_topn(q, topn), single.query_row_topn(q, topn)
                    assert a[0].tolist() == b[0].tolist() and a[1].tobytes() == b[1].tobytes()
        for name, rows, new in adversarial_steps(cur, q, 10, rng):
            cur[rows] = new
            nd.update_rows(rows, new)
            check_routes(nd, cur, q, f"{placement} {name}", labels, priors, batches=(12,))
        for bad in ([3, 3], [n], [-1]):
            with pytest.raises(capi.Mi355Error) as e:
                nd.update_rows(bad, rng.random((len(bad), 12), dtype=np.float32))
            assert e.value.code == capi.ERR_INVALID_ARG
        with pytest.raises(capi.Mi355Error) as e:
            nd.update_rows([1], None)                          # NULL rows on a node handle
        assert e.value.code == capi.ERR_INVALID_ARG
        check_routes(nd, cur, q, f"{placement} after the refused calls", labels, priors, batches=(2,))


def test_tickets_from_before_an_update_see_the_old_rows(capi, torch_cuda):
    """Two replicas on one device are lanes with streams of their own: the scans of an open window are still in flight when the
    update arrives, and it must not write under them.  2 097 153 rows make a scan long enough to be running; the rows written are
    the query's own best ten, so an answer that saw any of them written matches neither matrix."""
    from oracle import oracle
    from spotify_recommender_amd.engine import NodeEngine
    n = N_BUCKET
    cur = np.random.default_rng(n + 10).random((n, 12), dtype=np.float32)
    q = n // 3
    s_old = oracle.scores(cur, cur[q], threads=0)
    want_i, want_s = oracle.topn_canonical(s_old, q, 10)
    rows = [int(r) for r in want_i]
    new = np.repeat(-cur[q][None, :], len(rows), axis=0)
    with NodeEngine(cur, devices=[0, 0], placement=capi.PLACEMENT_REPLICATED) as nd:
        for _ in range(3):
            tickets = [nd.enqueue_row(q, 10) for _ in range(6)]
            nd.update_rows(rows, new)
            for t in tickets:
                idx, sc = nd.wait(t, 10)
                assert idx.tolist() == want_i.tolist(), "a ticket from before the update did not see the old rows"
                assert np.array_equal((sc + np.float32(0)).view(np.uint32), (want_s + np.float32(0)).view(np.uint32))
            nd.update_rows(rows, cur[rows])                    # back to the old rows for the next round
        cur[rows] = new
        nd.update_rows(rows, new)
        check_single(nd.query_row_topn(q, 10), cur, cur[q], q, 10, "after the update")


def test_refusals_leave_the_handle_as_it_was(Engine, capi, torch_cuda):
    n = 2049
    cur = catalogue(n)
    rng = np.random.default_rng(n + 8)
    labels, priors = side_data(n)
    q = n // 3
    with make(Engine, capi, cur, True) as eng:
        eng.set_labels(labels)
        eng.set_priors(priors)
        run = streamed_by_row(eng, torch_cuda)
        for bad in ([5, 9, 5], [5] + list(range(100, 400)) + [5], [0, n], [n - 1, -1]):   # duplicates (sorted and bitmap check), n, negative
            with pytest.raises(capi.Mi355Error) as e:
                eng.update_rows(bad, rng.random((len(bad), 12), dtype=np.float32))
            assert e.value.code == capi.ERR_INVALID_ARG
        assert eng.update_info()["calls"] == 0
        check_routes(eng, cur, q, "after the refused calls", labels, priors, run)
