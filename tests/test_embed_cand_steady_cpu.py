"""The candidate gather's STEADY STATE without a GPU (tests/embed_cand_steady_cases.py): the gather's list rules found in its
sources, the model's rounds and peaks at the gather's tile sizes, and every case's list — what workgroup b meets per round
(`landing`) is what the case intends, every rising, falling, fullest and plateau case compacts at least twice inside the
loop and stays inside the list's capacity, a FULLEST case reaches exactly kCandLimit - 1 + t.  Bit for bit on a few cases:
the list's reference answer (tests/test_gpu_embed_cand._oracle_rank) against the quick top-N, and `landing` against
csrc/embed_cand_request.h's claim_list through the stand-alone tests/embed_cand_check.cpp (AddressSanitizer and UBSan, its
own process)."""
import subprocess

import numpy as np
import pytest

from tests import embed_cand_steady_cases as cs
from tests import embed_oracle as eo
from tests import embed_steady_cases as sc
from tests.test_embed_cand_cpu import embed_cand_check  # noqa: F401  (the fixture that builds the program)
from tests.test_gpu_embed_cand import _oracle_rank

F32 = np.float32
K = cs.constants()
TOPNS = (1, 2, 10, 16, 63, 64, 127, 128, 129, 257, 511, 512, 513, 1000, 1023, 1024)   # test_no_case_of_any_size_exceeds_a_capacity's


def test_the_gather_states_the_scan_s_rules_and_the_model_gives_the_rounds():
    tiles = {(s, d): (cs.layout_of(s, d).tile_rows, cs.layout_of(s, d).capacity) for s in cs.STORAGES for d in cs.DIMS}
    assert [tiles[("f32", d)] for d in cs.DIMS] == [(512, 2560), (256, 2560), (128, 2560), (64, 2560)]
    assert [tiles[("fp16", d)] for d in cs.DIMS] == [(1024, 3072), (512, 3072), (256, 3072), (128, 3072)]
    assert [tiles[("bf16", d)] for d in cs.DIMS] == [tiles[("fp16", d)] for d in cs.DIMS]
    # the rounds after which a rising list has compacted twice: (top-10, top-257, top-1024) per tile size
    rounds = {cs.layout_of(s, d).tile_rows: tuple(sc.min_rounds(cs.layout_of(s, d), topn) for topn in (10, 257, 1024)) for s, d in tiles}
    assert rounds == {1024: (4, 4, 4), 512: (4, 4, 6), 256: (4, 5, 12), 128: (4, 8, 24), 64: (8, 14, 48)}
    # a table of G tiles runs G workgroups when the device has them, and the gather as many as its list has tiles
    for t in rounds:
        G = cs.ROWS // t
        assert G <= cs.MAX_GRID and cs.table_grid(cs.ROWS, t, 256) == G and cs.table_grid(cs.ROWS, t, 32) == G
        assert cs.table_grid(cs.ROWS, t, 1) == 2 and cs.table_grid(0, t, 256) == 1
        assert cs.gather_grid(1, t, G) == 1 and cs.gather_grid(G * t, t, G) == G and cs.gather_grid(50 * G * t + 1, t, G) == G
    assert cs.free_slots(64, 64, 5, 8) == (8 * 64 + 5 - 8) * 64 + 33


def test_no_list_of_full_tiles_of_any_length_exceeds_the_capacity():
    for storage in ("f32", "fp16"):
        for d in cs.DIMS:
            layout = cs.layout_of(storage, d)
            for topn in TOPNS:
                got = sc.occupancy(layout, [layout.tile_rows] * 300, topn)
                assert got["compactions"] >= 2 and got["peak"] <= layout.capacity and got["sort_room"] <= layout.capacity, (storage, d, topn, got)


def test_steady_list_and_landing_on_a_small_grid():
    n, t, G, b = 40, 4, 3, 2
    rounds_rows = [[5, 6, 7, 8], [9, 10], [11, 12, 13, 14]]
    slots = cs.free_slots(t, G, b, 3)
    assert slots == (3 * 3 + 2 - 3) * 4 + 3
    filler = np.concatenate([[0, 1, 2, 3, 4, 5, 40, -1, 2 ** 40], np.full(slots - 9, -7)])   # (5 is listed a second time: the first entry counts)
    ids = cs.steady_list(n, t, G, b, rounds_rows, filler)
    assert ids.size == (3 * 3 + 2) * 4 + 3
    tiles = [ids[i * t: (i + 1) * t].tolist() for i in range(12)]
    assert tiles[2] == [5, 6, 7, 8] and tiles[5] == [9, 10, -1, -1] and tiles[8] == [11, 12, 13, 14] and tiles[11] == [-7, -7, -7]
    assert tiles[0] == [0, 1, 2, 3] and tiles[1] == [4, 5, 40, -1] and tiles[3][0] == 2 ** 40
    v = np.arange(n, dtype=F32)
    v[[1, 10]] = np.nan
    land = cs.landing(ids, v, n, 0, t, G)
    assert land.shape == (G, 4) and land.tolist() == [[3, 0, 0, 0], [2, 0, 0, 0], [3, 1, 4, 0]]
    assert cs.landing(ids + 1000, v, n, 1000, t, G).tolist() == land.tolist()
    assert cs.landing(ids, v, n, 1000, t, G).sum() == 0, "local rows are not global ids"
    assert cs.claimed_rows(ids, n, 0).tolist() == list(range(15))


@pytest.mark.parametrize("case", cs.CASES, ids=cs.case_id)
def test_a_case_is_the_one_the_model_was_run_on(case):
    family, storage, d, what = case
    o = cs.build(case)
    t, G, b, L = o.t, o.G, o.b, K["kCandLimit"]
    assert o.n == G * t == cs.ROWS and G <= cs.MAX_GRID and b == cs.CASES.index(case) % G
    assert cs.list_shape(o) == (o.rounds * G + b + 1, G) and o.ids.size == (o.rounds * G + b) * t + t // 2 + 1
    land = cs.landing(o.ids, o.v, o.n, 0, t, G)
    mine = np.concatenate([np.asarray(r, np.int64) for r in o.rounds_rows])
    rows, counts = np.unique(o.ids[(o.ids >= 0) & (o.ids < o.n)], return_counts=True)
    assert rows.size == o.n, "every row of the table is listed"
    for w in range(G):   # no workgroup's list passes its capacity
        got = sc.occupancy(o.layout, land[w], max(o.topns))
        assert got["peak"] <= o.layout.capacity and got["sort_room"] <= o.layout.capacity, (w, got)
    if family == "twice":
        assert np.all(counts[mine] == 2) and counts.sum() == o.n + mine.size
        tile_of = np.nonzero(np.isin(o.ids, mine))[0] // t
        assert np.sum(tile_of % G == b) == mine.size, "the second copies lie in the tiles of other workgroups"
        assert cs.landing(o.ids_alone, o.v, o.n, 0, t, G)[b].tolist() == o.intended
        return
    assert np.all(counts == 1), "every row of the table is listed once: the claim is deterministic"
    assert land[b].tolist() == o.intended, (land[b].tolist(), o.intended)
    assert cs.landing(o.ids_alone, o.v, o.n, 0, t, G).sum() == sum(o.intended) and cs.landing(o.ids_alone, o.v, o.n, 0, t, G)[b].tolist() == o.intended
    for topn in o.topns:
        got = cs.model(o, topn=topn)
        assert got["compactions"] >= 2, (topn, got)
        assert got["peak"] <= o.layout.capacity and got["sort_room"] <= o.layout.capacity, (topn, got)
    vb = o.v[mine]
    if family == "rising":
        assert o.rounds == sc.min_rounds(o.layout, o.req["topn"]) and all(len(r) == t for r in o.rounds_rows)
        assert np.all(np.diff(vb.astype(np.float64)) >= 0), "rising across and within the rounds"
        assert vb.min() >= np.delete(o.v, mine).max() if mine.size < o.n else True, "workgroup b holds the best rows"
        neg = eo.values(o.wide, o.req["user"], eo.DOT if o.req["metric"] == "dot" else eo.COSINE, -o.req["embed_weight"],
                        -o.req.get("audio_weight", 0.0), o.feats, o.req.get("audio"))[0]
        assert np.array_equal(eo.bits(neg), eo.bits(-o.v)), "negated weights negate every v exactly: the falling case"
    if family == "fullest":
        got = cs.model(o)
        assert got["peak"] == L - 1 + t, got
        if d == 16:
            assert got["peak"] == o.layout.capacity - 1 == (2559 if storage == "f32" else 3071)
        short = o.intended.index(t - 1)
        assert len(o.rounds_rows[short]) == t - 1 + (what == "nan")
        assert sum(o.intended[:short + 1]) == L - 1 and o.intended[short + 1] == t
        assert np.all(np.diff(vb[np.isfinite(vb)].astype(np.float64)) >= 0)
        if what == "nan":
            assert o.nan_row == o.n - 1 and np.isnan(o.v[o.nan_row]) and int(np.isnan(o.v).sum()) == 1 and o.rounds_rows[short][-1] == o.nan_row
            cosine = eo.values(o.wide, o.req["user"], eo.COSINE, 1.0)[0]
            assert cosine[o.nan_row] == 0, "under cosine the row has a key: a later call must find its claim cleared"
        else:
            assert o.nan_row is None and np.all(np.isfinite(o.v)) and o.ids[(short * G + b) * t + t - 1] == -1
    if family == "plateau":
        flat = o.plateau
        assert flat.size == int(0.4 * o.n) and np.all(o.v[flat] == o.v.max()) and np.all(np.delete(o.v, flat) < o.v.max())
        first = L // t
        fed = np.concatenate(o.rounds_rows[first:])
        assert len(o.rounds_rows) - first >= 4 and fed.tolist() == flat[::-1].tolist(), "the plateau in falling id order over four rounds or more"
        assert np.all(np.diff(o.v[np.concatenate(o.rounds_rows[:first])].astype(np.float64)) >= 0)
        for topn in o.topns:
            assert eo.topn(o.v, topn)[0].tolist() == flat[:topn].tolist()


def _answers(o, req, ids, exclude=()):
    """(the reference as the GPU tests take it, the quick top-N over the same rows)."""
    v = cs._values(o.wide, o.feats, req)
    want = _oracle_rank(o, v, ids, dict(req, exclude=list(exclude)))
    only = np.full(o.n, np.nan, F32)
    rows = cs.claimed_rows(ids, o.n, o.row_base)
    only[rows] = v[rows]
    return want, sc.topn(only, req["topn"], exclude, o.row_base)


@pytest.mark.parametrize("case,row_base", [(cs.BASED, 0), (cs.BASED, 1_000_000), (("rising", "bf16", 128, "dot"), 0), (("fullest", "fp16", 16, "nan"), 0),
                                           (("plateau", "f32", 64, "cosine"), 0), (("twice", "f32", 16, "dot"), 0)],
                         ids=lambda x: cs.case_id(x) if isinstance(x, tuple) else str(x))
def test_the_reference_of_a_list_and_the_claim_statement(case, row_base, embed_cand_check, tmp_path):
    o = cs.build(case, row_base)
    for ids in (o.ids, o.ids_alone):
        for req in (o.req, cs.negated(o.req)):
            excl, _ = cs.exclusions(o, req, ids)
            assert len(excl) == 1024
            for exclude in ((), excl, [int(row_base + 5)], [5]):
                (wi, ws), (qi, qs) = _answers(o, req, ids, exclude)
                assert wi.tolist() == qi.tolist() and np.array_equal(eo.bits(ws), eo.bits(qs))
                assert wi.size > 0 and wi.min() >= row_base and not set(wi.tolist()) & set(exclude)
    # claim_list (sequential: the first entry of a row keeps it) names per tile what landing counts
    src, out = tmp_path / "ids.bin", tmp_path / "rows.bin"
    o.ids.tofile(src)
    p = subprocess.run([str(embed_cand_check), "claim", str(src), str(o.n), str(row_base), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = np.fromfile(out, np.uint32)
    assert rows.size == o.ids.size
    kept = rows != 0xFFFFFFFF
    assert np.sort(rows[kept]).tolist() == cs.claimed_rows(o.ids, o.n, row_base).tolist()
    assert np.array_equal(rows[kept].astype(np.int64) + row_base, o.ids[kept])
    tiles = -(-rows.size // o.t)
    rounds = -(-tiles // o.G)
    full = np.zeros(rounds * o.G * o.t, bool)
    full[: rows.size] = kept
    every = np.zeros(o.n, F32)   # (every row finite: landing counts what the claim keeps)
    assert np.array_equal(full.reshape(rounds, o.G, o.t).sum(axis=2).T, cs.landing(o.ids, every, o.n, row_base, o.t, o.G))
    if row_base:
        assert cs.landing(o.ids - row_base, every, o.n, row_base, o.t, o.G).sum() == 0
