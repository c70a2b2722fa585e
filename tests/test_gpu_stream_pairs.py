"""PAIRS of streamed single queries (mi355rec_set_stream_pairing; csrc/replica_q8.hip.h, scan_q8_kernel_pair): two queued
queries over the 8-bit replica with the same topn <= 128 are served by ONE pass over it.

Every case runs the same sequence of calls three ways — pairing ON, pairing OFF, and the CPU oracle (oracle.scores +
topn_canonical) — on handles with set_replica(ON), so that small shards take the 8-bit scan.  ON and OFF must agree key for
key, and both must equal the oracle in ids, order and score bits; every list of every case is compared in full.

The shapes are the smallest at which the pair form can go wrong: 5 rows (fewer rows than results), 2047 / 2049 (one row
short of a tile of 2048, one row into the second), 4099 (not a multiple of 4: the last quad is padding), 3 x 2048 + 1 (a
last partial tile-row); topn 1, 10, 128 and 129 (which must NOT pair); streams of 1, 2, 3, 4 and 7 queries (odd tails) —
and ONE case at the smallest row count at which a streamed launch has seed riders whose last one leaves a hoisted cutoff
(engine_state.hip.h, plan_replica: hoists = r_iters >= 5).
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from spotify_recommender_amd import capi

pytestmark = pytest.mark.gpu

FORMS7 = ("row", "row", "row", "value", "value", "pointer", "row")   # pairs: row + row, row + value, value + pointer; an odd tail


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def catalogue(n, seed):
    return np.random.default_rng(seed).random((n, 12), dtype=np.float32)


def make_calls(f, topns, forms, seed):
    """One call per entry of `topns`: {"form", "row", "vec", "exclude", "topn"}; by-value and by-pointer queries are fresh
    vectors that exclude nothing."""
    rng = np.random.default_rng(seed)
    n = f.shape[0]
    calls = []
    for i, topn in enumerate(topns):
        form = forms[i % len(forms)]
        row = int(rng.integers(0, n))
        if i == 0:
            row = n - 1   # (the last row: in the last, partial quad where n is no multiple of 4)
        vec = rng.random(12, dtype=np.float32) - np.float32(0.25)
        calls.append({"form": form, "row": row, "vec": vec, "exclude": row if form == "row" else -1, "topn": int(topn)})
    return calls


def issue(torch, eng, call, out, keep, stream=None):
    if call["form"] == "row":
        eng.enqueue_row_keys_streamed(call["row"], call["topn"], out, stream=stream)
    elif call["form"] == "value":
        eng.enqueue_query_keys_streamed(call["vec"], call["exclude"], call["topn"], out, stream=stream)
    else:
        dev = torch.from_numpy(call["vec"]).to("cuda")
        torch.cuda.synchronize()
        keep.append(dev)   # (the stream reads it up to three calls later)
        capi.check(eng._lib.mi355rec_enqueue_ptr_keys_streamed(
            eng._h, ctypes.c_void_p(dev.data_ptr()), call["exclude"], call["topn"], ctypes.c_void_p(out.data_ptr()),
            eng._stream_ptr(stream)), eng._h)


def run_stream(torch, f, calls, pairing, hooks=None):
    """The calls on a fresh handle over `f` (set_replica(ON)), hooks[i](eng) before call i; returns the raw key lists and
    the stats deltas {"q8", "pairs", "scans"}."""
    from spotify_recommender_amd.engine import CosineEngine, set_stream_pairing
    outs = [torch.zeros(c["topn"], dtype=torch.int64, device="cuda") for c in calls]
    keep = []
    torch.cuda.synchronize()
    with CosineEngine(f) as eng:
        eng.set_replica(capi.REPLICA_ON)
        set_stream_pairing(eng, pairing)
        before, scans0 = eng.stats(), eng.replica_counters()["scans"]
        for i, c in enumerate(calls):
            if hooks and i in hooks:
                hooks[i](eng, outs)
            issue(torch, eng, c, outs[i], keep)
        eng.enqueue_flush()
        torch.cuda.synchronize()
        after, scans1 = eng.stats(), eng.replica_counters()["scans"]
    books = {"q8": after.route_q8 - before.route_q8, "pairs": after.stream_pair_launches - before.stream_pair_launches,
             "scans": scans1 - scans0}
    return [o.cpu().numpy().copy() for o in outs], books


def query_of(f, call):
    return f[call["row"]] if call["form"] == "row" else call["vec"]


def want_keys(f, call):
    """(ids, scores) of the oracle for one call over the rows `f`."""
    s = oracle.scores(f, np.ascontiguousarray(query_of(f, call)), threads=0)
    return oracle.topn_canonical(s, call["exclude"], call["topn"])


def assert_list(keys, want, what):
    from spotify_recommender_amd.engine import unpack_keys
    want_i, want_s = want
    rows, sc = unpack_keys(keys)
    assert rows.tolist() == want_i.tolist(), f"{what}: ids {rows.tolist()[:8]} != {want_i.tolist()[:8]}"
    assert np.array_equal(sc.view(np.uint32), (want_s + np.float32(0)).view(np.uint32)), f"{what}: score bits"


def check_three_ways(torch, f, calls, hooks=None, rows_at=None, expect_pairs=None):
    """ON against OFF key for key, both against the oracle.  rows_at(i): the rows call i sees (a hook changed them)."""
    on, books_on = run_stream(torch, f, calls, capi.PAIRING_ON, hooks)
    off, books_off = run_stream(torch, f, calls, capi.PAIRING_OFF, hooks)
    for i, c in enumerate(calls):
        assert np.array_equal(on[i], off[i]), f"call {i} ({c['form']}, topn {c['topn']}): ON and OFF differ"
        want = want_keys(f if rows_at is None else rows_at(i), c)
        assert_list(on[i], want, f"ON, call {i} ({c['form']}, topn {c['topn']})")
        assert_list(off[i], want, f"OFF, call {i} ({c['form']}, topn {c['topn']})")
    assert books_off["pairs"] == 0
    if expect_pairs is not None:
        assert books_on["pairs"] == expect_pairs, books_on
    return books_on, books_off


# ---- sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topn", [1, 10, 128, 129])
@pytest.mark.parametrize("n", [5, 2047, 2049, 4099, 3 * 2048 + 1])
def test_rows_and_topn(torch_cuda, n, topn):
    f = catalogue(n, 1000 + n)
    calls = make_calls(f, [topn] * 7, FORMS7, n + topn)
    on, off = check_three_ways(torch_cuda, f, calls, expect_pairs=0 if topn > 128 else 3)
    # the books stay per QUERY: seven launches' worth of queries either way
    assert on["q8"] == 7 and off["q8"] == 7 and on["scans"] == 7 and off["scans"] == 7, (on, off)


@pytest.mark.parametrize("count", [1, 2, 3, 4, 7])
def test_queries_per_stream(torch_cuda, count):
    f = catalogue(4099, 77)
    calls = make_calls(f, [10] * count, FORMS7, count)
    on, off = check_three_ways(torch_cuda, f, calls, expect_pairs=count // 2)
    assert on["q8"] == count and off["q8"] == count, (on, off)


# ---- special pairs, invalid partners, special rows ------------------------------------------------------------------
def test_identical_partners_and_a_partner_that_excludes_the_others_row(torch_cuda):
    f = catalogue(4099, 5)
    a = {"form": "row", "row": 1234, "vec": f[1234].copy(), "exclude": 1234, "topn": 10}
    b = {"form": "value", "row": 77, "vec": f[77].copy(), "exclude": 1234, "topn": 10}   # excludes A's query row, not its own
    check_three_ways(torch_cuda, f, [a, dict(a), a, b, b, a], expect_pairs=3)


@pytest.mark.parametrize("bad", ["zero", "nan"])
def test_an_invalid_partner_leaves_the_other_alone(torch_cuda, bad):
    f = catalogue(4099, 6)
    vec = np.zeros(12, dtype=np.float32)
    if bad == "nan":
        vec = f[9].copy()
        vec[5] = np.nan
    good = {"form": "row", "row": 4000, "vec": f[4000].copy(), "exclude": 4000, "topn": 10}
    invalid = {"form": "value", "row": 0, "vec": vec, "exclude": -1, "topn": 10}
    check_three_ways(torch_cuda, f, [good, invalid, invalid, good], expect_pairs=2)


def test_a_zero_row_and_a_nan_row_in_the_catalogue(torch_cuda):
    f = catalogue(4099, 7)
    f[3] = 0.0
    f[4097, 2] = np.nan
    calls = make_calls(f, [10, 10, 128, 128], ("row", "value"), 8)
    calls[1]["form"], calls[1]["row"], calls[1]["exclude"] = "row", 3, 3   # the zero row as a query, too
    check_three_ways(torch_cuda, f, calls, expect_pairs=2)


# ---- state changes between the calls of a pair -----------------------------------------------------------------------
def test_topn_changes_mid_stream(torch_cuda):
    f = catalogue(6145, 9)
    calls = make_calls(f, [10, 10, 10, 100, 100, 1, 1, 129, 10], FORMS7, 10)
    # (10, 10) pairs; the third 10 finds no partner; (100, 100) and (1, 1) pair; 129 and the last 10 go alone
    check_three_ways(torch_cuda, f, calls, expect_pairs=3)


def test_set_replica_between_the_calls_of_a_pair(torch_cuda):
    f = catalogue(6145, 11)
    calls = make_calls(f, [10] * 6, FORMS7, 12)
    hooks = {1: lambda eng, outs: eng.set_replica(capi.REPLICA_OFF), 3: lambda eng, outs: eng.set_replica(capi.REPLICA_ON)}
    # call 0 waits for a partner that takes the fp32 rows; calls 1, 2 scan the fp32 rows; 3 + 4 pair; 5 is the odd tail
    on, off = check_three_ways(torch_cuda, f, calls, hooks=hooks, expect_pairs=1)
    assert on["q8"] == 4 and off["q8"] == 4, (on, off)


def test_update_rows_between_the_calls_of_a_pair(torch_cuda):
    f = catalogue(4099, 13)
    calls = make_calls(f, [10] * 5, ("row", "value"), 14)
    changed = np.array([calls[0]["row"], 17, 2050], dtype=np.int64)
    fresh = catalogue(3, 15)
    f_new = f.copy()
    f_new[changed] = fresh
    hooks = {1: lambda eng, outs: eng.update_rows(changed, fresh)}
    # the update closes the stream first: call 0 sees the old rows (alone), calls 1.. the new ones (1 + 2 and 3 + 4 pair)
    check_three_ways(torch_cuda, f, calls, hooks=hooks, rows_at=lambda i: f if i == 0 else f_new, expect_pairs=2)


def test_a_synchronous_query_in_between_flushes_the_stream(torch_cuda):
    torch = torch_cuda
    f = catalogue(4099, 16)
    calls = make_calls(f, [10] * 4, ("row", "value"), 17)
    sync_want = oracle.topn_canonical(oracle.scores(f, f[5], threads=0), 5, 10)
    seen = {}

    def sync_query(eng, outs):
        idx, sc = eng.query_row_topn(5, 10)
        assert idx.tolist() == sync_want[0].tolist() and np.array_equal(sc, sync_want[1] + np.float32(0))
        torch.cuda.synchronize()
        seen[len(seen)] = outs[0].cpu().numpy().copy()   # call 0's keys, with no flush of the caller's

    on, _ = check_three_ways(torch, f, calls, hooks={1: sync_query}, expect_pairs=1)
    # run 0 is the pairing-ON one: the synchronous call did not leave call 0 waiting for a partner across it
    assert_list(seen[0], want_keys(f, calls[0]), "call 0 right after the synchronous query")


# ---- lanes ------------------------------------------------------------------------------------------------------------
def test_two_lanes_with_ring_buffers(torch_cuda):
    """Sixteen queries dealt alternately over a handle and its lane, each on its own stream, four ring buffers per lane
    re-used: a buffer ends with the keys of the LAST query that was given it — the keys are written in call order."""
    torch = torch_cuda
    from spotify_recommender_amd.engine import CosineEngine, set_stream_pairing
    f = catalogue(6145, 18)
    rows = [int(r) for r in np.random.default_rng(19).integers(0, f.shape[0], size=16)]
    final = {}
    for mode in (capi.PAIRING_ON, capi.PAIRING_OFF):
        with CosineEngine(f) as eng:
            eng.set_replica(capi.REPLICA_ON)
            set_stream_pairing(eng, mode)   # (before the lane is made: it inherits the mode)
            lane = eng.lane()
            pair, streams = [eng, lane], [eng.own_stream(), lane.own_stream()]
            rings = [[torch.zeros(10, dtype=torch.int64, device="cuda") for _ in range(4)] for _ in pair]
            torch.cuda.synchronize()
            before = [e.stats().stream_pair_launches for e in pair]
            for k, r in enumerate(rows):
                pair[k % 2].enqueue_row_keys_streamed(r, 10, rings[k % 2][(k // 2) % 4], stream=streams[k % 2])
            for e, s in zip(pair, streams):
                e.enqueue_flush(stream=s)
            torch.cuda.synchronize()
            launches = [e.stats().stream_pair_launches - b for e, b in zip(pair, before)]
            assert launches == ([4, 4] if mode == capi.PAIRING_ON else [0, 0]), launches
            final[mode] = [[b.cpu().numpy().copy() for b in ring] for ring in rings]
            lane.close()
    for ln in range(2):
        for slot in range(4):
            k = 8 + 2 * slot + ln   # the last query dealt to this lane's buffer `slot`
            want = oracle.topn_canonical(oracle.scores(f, f[rows[k]], threads=0), rows[k], 10)
            assert np.array_equal(final[capi.PAIRING_ON][ln][slot], final[capi.PAIRING_OFF][ln][slot]), (ln, slot)
            assert_list(final[capi.PAIRING_ON][ln][slot], want, f"ON, lane {ln}, buffer {slot}")
            assert_list(final[capi.PAIRING_OFF][ln][slot], want, f"OFF, lane {ln}, buffer {slot}")


# ---- riders and a hoisted cutoff ----------------------------------------------------------------------------------------
# plan_replica (engine_state.hip.h): a full grid is 2 workgroups per CU (512 on 256 CUs); a streamed launch then has
# min(grid / 8, 256 regions / 4) = 64 riders and r_scan = grid - 2 - riders = 446 scanners, and the last rider leaves the
# cutoff (hoists) from r_iters = ceil(tiles / r_scan) >= 5 on: tiles = 4 * 446 + 1 = 1785 tiles of 2048 rows.
RIDER_GRID = 512
RIDER_ROWS = (4 * (RIDER_GRID - 2 - RIDER_GRID // 8)) * 2048 + 1   # 3 653 633


@pytest.fixture(scope="module")
def big(torch_cuda):
    f = catalogue(RIDER_ROWS, 20)
    calls = make_calls(f, [10] * 6, FORMS7, 21)
    return f, calls, [want_keys(f, c) for c in calls]


def run_big(torch, f, calls, pairing, hooks=None):
    from spotify_recommender_amd.engine import CosineEngine, set_stream_pairing
    outs = [torch.zeros(c["topn"], dtype=torch.int64, device="cuda") for c in calls]
    keep = []
    torch.cuda.synchronize()
    with CosineEngine(f) as eng:
        assert eng.stats().replica_grid_blocks == RIDER_GRID, "RIDER_ROWS was worked out for a grid of 512 workgroups"
        set_stream_pairing(eng, pairing)
        before = eng.stats().stream_pair_launches
        for i, c in enumerate(calls):
            if hooks and i in hooks:
                hooks[i](eng)
            issue(torch, eng, c, outs[i], keep)
        eng.enqueue_flush()
        torch.cuda.synchronize()
        pairs = eng.stats().stream_pair_launches - before
    return [o.cpu().numpy().copy() for o in outs], pairs


@pytest.mark.parametrize("sample", ["auto", "toggled"])
def test_riders_and_a_hoisted_cutoff(torch_cuda, big, sample):
    """Six queries at the smallest shard whose streamed launches carry riders and a hoisted cutoff; `toggled` also changes
    mi355rec_set_sample between the calls of a pair (BUCKETED before call 1, STRIDED before call 4)."""
    f, calls, wants = big
    hooks = None
    if sample == "toggled":
        hooks = {1: lambda eng: eng.set_sample(capi.SAMPLE_BUCKETED), 4: lambda eng: eng.set_sample(capi.SAMPLE_STRIDED)}
    on, pairs_on = run_big(torch_cuda, f, calls, capi.PAIRING_ON, hooks)
    off, pairs_off = run_big(torch_cuda, f, calls, capi.PAIRING_OFF, hooks)
    # (toggled: call 0 loses its partner to the change before call 1, 1 + 2 pair, 3 loses its partner to the second change, 4 + 5 pair)
    assert (pairs_on, pairs_off) == ((3, 0) if sample == "auto" else (2, 0))
    for i, c in enumerate(calls):
        assert np.array_equal(on[i], off[i]), f"call {i}: ON and OFF differ"
        assert_list(on[i], wants[i], f"ON, call {i} ({c['form']})")
        assert_list(off[i], wants[i], f"OFF, call {i} ({c['form']})")
