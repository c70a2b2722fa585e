"""The pair kernel's tile loop (csrc/replica_q8.hip.h, scan_q8_kernel_pair): a lane's tile addresses run on from tile to tile
by a stride and are clamped past the last quad, the unrolled loop stops at any `iters`, a wave asks "does any row reach either
cut" before it works out which (q8_pair_excess4), and the rows found are fetched into a slot both queries share and scored one
tile later.  What can go wrong depends on `iters`, the tiles a scanning workgroup sees — its residue modulo the ring decides
where the loop stops and which tile the final consume belongs to, iters = 1 must not score the prefetched tile — and on where in
a quad, a tile and the catalogue the candidates lie.

`iters` is the host's (csrc/engine_single.hip.h, launch_pairs; csrc/engine_state.hip.h, plan_replica), modelled below for a chip
of 256 CUs holding two workgroups of the scan per CU:

    tiles = ceil(n / 2048);  grid = min(tiles, 512);  riders = min(ceil(min(n // 2048, 256) / 4), grid // 8) where grid >= 16
    side  = 4 where the launch scans for two pairs, merges four lists or carries four queries after, else 2
    extra = side * (1 + (riders + 1 where the launch carries queries after and riders > 0))
    slots = two pairs: (512 - extra) // 2, one pair: grid - extra; at most `tiles`, two pairs from 8 up a multiple of 8, at least 1
    iters = ceil(tiles / slots)

and which launches a stream makes is modelled from the rules of include/mi355rec_diag.h (a group closes at four queries, at two
where the handle forms pairs only or a query by pointer is in the group or waits for its launch; the flush closes the complete
pair it finds).  Every case states the (pairs, iters) of its launches under GROUPS and ON; the model must give exactly those, the
engine's books must count exactly those launches, and together the cases show a pair launch and a launch for two pairs iters of
1, 2, 3, 4, 5 and 7 each.

Every case runs GROUPS and ON against OFF key for key and against the CPU oracle in ids, order and score bits.  Queries 0 and 1
(one pair) are the SAME vector by value, and exact copies of it are planted at the first row of the last tile, at the last row
(the last valid quad: the final consume and the padding mask decide), at two rows of one quad and three rows of another (the
`rest` loop) — every planted row is a candidate of both queries of the pair (the shared pending slot)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from spotify_recommender_amd import capi

pytestmark = pytest.mark.gpu

TILE = 2048
CUS = 256   # what the stated iters assume; the test fails with a message on another chip
MODES = (("GROUPS", capi.PAIRING_GROUPS), ("ON", capi.PAIRING_ON), ("OFF", capi.PAIRING_OFF))


# ---- the host's arithmetic ------------------------------------------------------------------------------------------------
def launch_iters(n, pairs, n_next, n_pending, cus=CUS):
    tiles = -(-n // TILE)
    cap = min(2 * cus, 1024)
    grid = min(tiles, cap)
    siters = -(-tiles // (grid - 1 if grid > 1 else 1))
    regions = min(n // TILE, 256)
    riders = 0
    if regions > 0 and grid >= 16:
        rounds = max(1, int(siters * 2.1 / 12.0))
        riders = min(-(-regions // (4 * rounds)), grid // 8)
    side = 4 if (pairs == 2 or n_pending == 4 or n_next == 4) else 2
    extra = side * (1 + (riders + 1 if n_next > 0 and riders > 0 else 0))
    slots = (cap - extra) // 2 if pairs == 2 else grid - extra
    slots = min(slots, 1023, tiles)
    if pairs == 2 and slots >= 8:
        slots &= ~7
    slots = max(slots, 1)
    return -(-tiles // slots)


def stream_launches(forms, groups):
    """[(pairs, queries after, lists to merge)] of the launches of a stream of calls closed by a flush."""
    form, wait, out = [], [], []
    pending = 0

    def launch(n_next):
        nonlocal pending
        out.append((len(wait) // 2, n_next, pending))
        pending = len(wait)

    def close(k):
        if wait:
            launch(k)
        wait[:] = form[:k]
        del form[:k]

    for f in forms:
        form.append(f)
        if len(form) % 2:
            continue
        if len(form) == 4 or not groups or "pointer" in form + wait:
            close(len(form))
    if len(form) >= 2:
        close(2)
    if wait:
        launch(0)
    return out


def pairs_and_iters(n, forms, groups, cus=CUS):
    return [(p, launch_iters(n, p, nn, pend, cus)) for p, nn, pend in stream_launches(forms, groups)]


R6 = ("value", "value", "row", "value", "row", "row")
POINTER = ("value", "value", "row", "row", "pointer", "row", "row", "value")   # a group, then pairs: (p r) closes at two, and so does the pair behind it

# name: (rows, forms, topn, launches under GROUPS, launches under ON) — launches as (pairs, iters), in order
CASES = {
    # one tile: the prologue's second tile is the clamped one and must not be scored
    "1 tile": (1501, R6, 10, [(2, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]),
    "1 tile, 1 row": (1, R6, 10, [(2, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]),
    # 2 .. 5 tiles: no riders, slots = tiles - extra or 1; the pair behind a group merges four lists (extra 4)
    "2 tiles": (TILE + 1, R6, 10, [(2, 1), (1, 2)], [(1, 2), (1, 2), (1, 2)]),
    "3 tiles": (2 * TILE + 1, R6, 10, [(2, 1), (1, 3)], [(1, 3), (1, 3), (1, 3)]),
    "4 tiles": (3 * TILE + 2, R6, 10, [(2, 1), (1, 4)], [(1, 2), (1, 2), (1, 2)]),
    "5 tiles": (4 * TILE + 2047, R6, 10, [(2, 1), (1, 5)], [(1, 2), (1, 2), (1, 2)]),
    # 9 tiles: two pairs get 8 slots each
    "9 tiles": (8 * TILE + 3, R6, 10, [(2, 2), (1, 2)], [(1, 2), (1, 2), (1, 2)]),
    # 19 tiles, riders: the pair launch behind a group has 4 x (1 + 2 + 1) = 16 workgroups that do not scan, 3 that do
    "19 tiles": (18 * TILE + 1, POINTER, 10, [(2, 2), (1, 7), (1, 2)], [(1, 2), (1, 2), (1, 2), (1, 2)]),
    # two pairs at (512 - 4 x (2 + riders)) // 2 slots, rounded down to 8: 160, 136, 120, 120 slots
    "344 tiles": (343 * TILE + 1, R6, 10, [(2, 3), (1, 2)], [(1, 2), (1, 2), (1, 2)]),
    "440 tiles": (439 * TILE + 2047, R6, 10, [(2, 4), (1, 2)], [(1, 2), (1, 2), (1, 2)]),
    "504 tiles": (503 * TILE + 2, R6, 100, [(2, 5), (1, 2)], [(1, 2), (1, 2), (1, 2)]),
    "728 tiles": (727 * TILE + 3, R6, 10, [(2, 7), (1, 2)], [(1, 2), (1, 2), (1, 2)]),
}


def test_the_stated_iters_are_the_hosts_and_cover_every_residue(torch_cuda):
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert cus == CUS, f"the cases' row counts were chosen for a chip of {CUS} CUs, this one has {cus}"
    seen = {1: set(), 2: set()}
    for name, (n, forms, _, groups, on) in CASES.items():
        assert pairs_and_iters(n, forms, True, cus) == groups, (name, pairs_and_iters(n, forms, True, cus))
        assert pairs_and_iters(n, forms, False, cus) == on, (name, pairs_and_iters(n, forms, False, cus))
        for p, it in groups + on:
            seen[p].add(it)
    assert seen[1] >= {1, 2, 3, 4, 5, 7} and seen[2] >= {1, 2, 3, 4, 5, 7}, seen
    at_three_up = [n for n, _, _, groups, on in CASES.values() if max(it for _, it in groups + on) >= 3]
    assert {n % 4 for n in at_three_up} >= {1, 2, 3} and {n % TILE for n in at_three_up} >= {1, 2047}


# ---- the streams ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def planted(n):
    """Rows that hold exact copies of row 0 (where the catalogue has them)."""
    last_tile = (n - 1) // TILE * TILE
    mid = (n // 2) & ~3
    rows = [last_tile, n - 1, mid, mid + 1, mid + 9, mid + 10, mid + 11]
    return sorted({r for r in rows if 0 < r < n})


def build_case(n, forms, topn, seed):
    rng = np.random.default_rng(seed)
    f = rng.random((n, 12), dtype=np.float32)
    f[planted(n)] = f[0]
    calls = []
    for i, form in enumerate(forms):
        row = 0 if i < 3 else int(rng.integers(0, n))
        vec = f[0].copy() if i < 2 else rng.random(12, dtype=np.float32) - np.float32(0.25)
        calls.append({"form": form, "row": row, "vec": vec, "exclude": row if form == "row" else -1, "topn": topn})
    return f, calls


def run_stream(torch, f, calls, pairing):
    from spotify_recommender_amd.engine import CosineEngine, set_stream_pairing
    outs = [torch.zeros(c["topn"], dtype=torch.int64, device="cuda") for c in calls]
    keep = []
    for c in calls:
        if c["form"] == "pointer":
            keep.append(torch.from_numpy(c["vec"]).to("cuda"))
    torch.cuda.synchronize()
    with CosineEngine(f) as eng:
        eng.set_replica(capi.REPLICA_ON)
        set_stream_pairing(eng, pairing)
        before = eng.stats()
        devs = iter(keep)
        for c, o in zip(calls, outs):
            if c["form"] == "row":
                eng.enqueue_row_keys_streamed(c["row"], c["topn"], o)
            elif c["form"] == "value":
                eng.enqueue_query_keys_streamed(c["vec"], c["exclude"], c["topn"], o)
            else:
                capi.check(eng._lib.mi355rec_enqueue_ptr_keys_streamed(
                    eng._h, ctypes.c_void_p(next(devs).data_ptr()), c["exclude"], c["topn"], ctypes.c_void_p(o.data_ptr()),
                    eng._stream_ptr(None)), eng._h)
        eng.enqueue_flush()
        torch.cuda.synchronize()
        after = eng.stats()
    books = (after.route_q8 - before.route_q8, after.stream_pair_launches - before.stream_pair_launches,
             after.stream_group_launches - before.stream_group_launches)
    return [o.cpu().numpy().copy() for o in outs], books


def check_case(torch, f, calls, launches_groups, launches_on):
    from spotify_recommender_amd.engine import unpack_keys
    got = {}
    for name, mode in MODES:
        got[name], books = run_stream(torch, f, calls, mode)
        launches = {"GROUPS": launches_groups, "ON": launches_on, "OFF": []}[name]
        want_books = (len(calls), sum(p for p, _ in launches), sum(1 for p, _ in launches if p == 2))
        assert books == want_books, (name, books, want_books)
    wants = {}
    for i, c in enumerate(calls):
        q = f[c["row"]] if c["form"] == "row" else c["vec"]
        key = (q.tobytes(), c["exclude"])
        if key not in wants:
            wants[key] = oracle.topn_canonical(oracle.scores(f, np.ascontiguousarray(q), threads=0), c["exclude"], c["topn"])
        want_i, want_s = wants[key]
        for name, _ in MODES:
            assert np.array_equal(got[name][i], got["OFF"][i]), f"call {i}: {name} and OFF differ"
            rows, sc = unpack_keys(got[name][i][:len(want_i)])
            assert rows.tolist() == want_i.tolist(), f"{name}, call {i}: ids {rows.tolist()[:8]} != {want_i.tolist()[:8]}"
            assert np.array_equal(sc.view(np.uint32), (want_s + np.float32(0)).view(np.uint32)), f"{name}, call {i}: score bits"
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_iters(torch_cuda, name):
    n, forms, topn, launches_groups, launches_on = CASES[name]
    f, calls = build_case(n, forms, topn, 2900 + len(name) + n % 97)
    got = check_case(torch_cuda, f, calls, launches_groups, launches_on)
    if n > 16:   # the planted copies lead both lists of the pair (equal scores: the lower row first)
        from spotify_recommender_amd.engine import unpack_keys
        copies = ([0] + planted(n))[:topn]
        for i in (0, 1):
            assert unpack_keys(got["GROUPS"][i])[0].tolist()[:len(copies)] == copies, (name, i)


def test_a_query_without_a_bound_beside_one_with(torch_cuda):
    """The zero vector has no 8-bit image: its cut_d is INT_MIN, "every row is a candidate" — the excess is then measured
    against the clamped cut (q8_pair_neg_cut) and must be >= 0 for every row, while its partner in the pair keeps its own cut."""
    n = 2 * TILE + 1
    f, calls = build_case(n, R6, 10, 2931)
    calls[1] = {"form": "value", "row": 0, "vec": np.zeros(12, dtype=np.float32), "exclude": -1, "topn": 10}
    calls[4] = dict(calls[1])
    check_case(torch_cuda, f, calls, [(2, 1), (1, 3)], [(1, 3)] * 3)


def test_a_workgroup_compacts_in_the_middle_of_its_scan(torch_cuda):
    """5 tiles, 3 000 rows within 0.2 % of one vector, top-100: the last pair of the stream is scanned by ONE workgroup (iters 5
    under GROUPS; 3 slots, iters 2 under ON) whose 8-bit cutoff lets hundreds of rows per tile through, so it passes compact_at
    (256 candidates) after its first tiles and tightens — cut_d moves, and with it what the excess is measured against — with
    the ring's tiles live."""
    n = 4 * TILE + 2
    rng = np.random.default_rng(2929)
    f = rng.random((n, 12), dtype=np.float32)
    centre = f[7].copy()
    near = rng.choice(n, size=3000, replace=False)
    f[near] = (centre * (1.0 + rng.normal(0.0, 0.002, (3000, 12)))).astype(np.float32)
    f[7] = centre
    forms = ("row", "value", "row", "value", "value", "row")
    calls = []
    for i, form in enumerate(forms):
        row = 7 if i in (1, 4, 5) else int(near[i])
        vec = centre.copy() if i in (1, 4) else f[row].copy()
        calls.append({"form": form, "row": row, "vec": vec, "exclude": row if form == "row" else -1, "topn": 100})
    assert pairs_and_iters(n, forms, True) == [(2, 1), (1, 5)] and pairs_and_iters(n, forms, False) == [(1, 2)] * 3
    check_case(torch_cuda, f, calls, [(2, 1), (1, 5)], [(1, 2)] * 3)
