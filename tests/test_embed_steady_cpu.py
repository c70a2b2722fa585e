"""The embedding scans' STEADY STATE without a GPU (tests/embed_steady_cases.py): the list-occupancy model over constants
read out of csrc/core.hip.h, csrc/embed.hip.h and csrc/embed_batch.hip.h — the bound cases reach a list's last slot and no
case passes it, every rising case compacts twice inside the tile loop — the builders (rising, holes, plateau, the quick
top-N), and the rising, falling and plateau tables at a few thousand rows against the CPU placement of the fp32 library
(the half and batch libraries have none), bit for bit through tests/embed_cases.check."""
import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_oracle as eo
from tests import embed_steady_cases as sc

F32 = np.float32
K = sc.constants()


def test_the_constants_are_the_sources():
    want = dict(kEmbedBlock=512, kEmbedVecsPerThread=4, kEmbedTileVecs=2048, kMaxTopK=1024, kCandLimit=2048, kEmbedBatchMaxTopK=128,
                kEmbedBatchCandLimit=256, kEmbedBatchMaxPass=8, kRankCountMax=160, kMergeMaxLists=2048, half_vals=8, f32_vals=4,
                slack_div=4, slack_min=16, compact_floor=256)
    assert {name: K.get(name) for name in want} == want
    # the tiles and capacities of the issue's table
    got = {(kind, d): (sc.Layout(kind, d, K).tile_rows, sc.Layout(kind, d, K).capacity) for kind in ("f32", "fp16", "batch") for d in sc.DIMS}
    assert got[("f32", 16)] == (512, 2560) and got[("f32", 128)] == (64, 2560)
    assert got[("fp16", 16)] == (1024, 3072) and got[("fp16", 128)] == (128, 3072)
    assert [got[("batch", d)] for d in sc.DIMS] == [(512, 768), (256, 512), (128, 384), (64, 320)]
    assert sc.grid_of(256, K) == 512 and sc.grid_of(2000, K) == 2048
    assert sc.sizes(512, 512, 4) == 4 * 512 * 512 + 257


@pytest.mark.parametrize("kind,d,topn,per_round,rounds,short", sc.BOUND_CASES)
def test_a_bound_case_reaches_the_last_slot_and_no_further(kind, d, topn, per_round, rounds, short):
    layout = sc.Layout(kind, d, K)
    assert len(per_round) == rounds and max(per_round) <= layout.tile_rows and topn == layout.max_topn
    got = sc.occupancy(layout, per_round, topn)
    assert got["peak"] == layout.capacity - short, got
    assert got["sort_room"] <= layout.capacity
    # workgroup 0 also scans the partial last tile
    tail = sc.occupancy(layout, per_round + [layout.tile_rows // 2 + 1], topn)
    assert tail["peak"] == got["peak"] and tail["sort_room"] <= layout.capacity
    # ... and through the builders, on a synthetic grid of 4
    grid = 4
    n = sc.sizes(layout.tile_rows, grid, rounds)
    mask = sc.holes(n, layout.tile_rows, grid, per_round)
    v = np.where(mask, np.nan, np.arange(n)).astype(F32)
    counts = sc.finite_counts(v, layout.tile_rows, grid)
    assert counts.shape == (grid, rounds + 1)
    assert np.array_equal(counts[:, :rounds], np.tile(per_round, (grid, 1)))
    assert counts[:, rounds].tolist() == [layout.tile_rows // 2 + 1, 0, 0, 0]
    assert sc.peaks(layout, v, grid, topn)[0] == layout.capacity - short


def test_the_peaks_of_the_table():
    peak = {(kind, d): sc.occupancy(sc.Layout(kind, d, K), per_round, topn)["peak"] for kind, d, topn, per_round, _, _ in sc.BOUND_CASES}
    assert peak == {("f32", 16): 2559, ("fp16", 16): 3071, ("bf16", 16): 3071, ("batch", 16): 768, ("batch", 32): 512, ("batch", 64): 384,
                    ("batch", 128): 320}
    # one row more in the short round would trigger a round early: the peak is the case's, not any table's
    assert sc.occupancy(sc.Layout("f32", 16, K), [512] * 6, 1024)["peak"] == 2304
    assert sc.occupancy(sc.Layout("batch", 16, K), [512] * 4, 128)["peak"] == 672


@pytest.mark.parametrize("kind,d,what,topns", sc.rising_cases())
def test_a_rising_case_compacts_twice_and_stays_inside(kind, d, what, topns):
    layout = sc.Layout(kind, d, K)
    rounds = sc.rising_rounds(kind, d, topns, K)
    assert rounds >= 4
    for topn in topns:
        for appends in ([layout.tile_rows] * rounds, [layout.tile_rows] * rounds + [layout.tile_rows // 2 + 1]):
            got = sc.occupancy(layout, appends, topn)
            assert got["compactions"] >= 2, (topn, got)
            assert got["peak"] <= layout.capacity and got["sort_room"] <= layout.capacity, (topn, got)


def test_no_case_of_any_size_exceeds_a_capacity():
    """The invariant itself, under the model: full tiles for ever, every topn a library serves."""
    for kind in ("f32", "fp16", "batch"):
        for d in sc.DIMS:
            layout = sc.Layout(kind, d, K)
            for topn in (1, 2, 10, 16, 63, 64, 127, 128, 129, 257, 511, 512, 513, 1000, 1023, 1024):
                if topn > layout.max_topn:
                    continue
                got = sc.occupancy(layout, [layout.tile_rows] * 40, topn)
                assert got["peak"] <= layout.capacity and got["sort_room"] <= layout.capacity, (kind, d, topn, got)


@pytest.mark.parametrize("storage", ["f32", "fp16", "bf16"])
def test_rising_is_non_decreasing_under_the_oracle(storage):
    from spotify_recommender_amd.embed_half import to_storage, widen
    n, d = 3001, 32
    feats, table = ec.catalogue(n, d)
    table = table[np.all(np.isfinite(table), axis=1)]
    table[20:40] = table[19]   # ties: the sort is stable
    feats = feats[: table.shape[0]]
    user = ec.requests(n, d)[0]["user"]
    stored = table if storage == "f32" else to_storage(table, storage)
    wide = table if storage == "f32" else widen(stored, storage)
    for metric in (eo.COSINE, eo.DOT):
        v, _ = eo.values(wide, user, metric, 1.0)
        ok = np.isfinite(v)   # (1e19 rows: inf under dot)
        out, vs, fs = sc.rising(stored[ok], v[ok], feats[ok])
        wide_out = out if storage == "f32" else widen(out, storage)
        again, _ = eo.values(wide_out, user, metric, 1.0)
        assert np.array_equal(eo.bits(again), eo.bits(vs)) and np.all(np.diff(again.astype(np.float64)) >= 0)
        assert ec.same_floats(eo.values(wide_out, user, metric, -1.0)[0], -again), "negated weights negate every v exactly: the falling case"
        order = np.argsort(v[ok], kind="stable")
        assert np.array_equal(fs, feats[ok][order]) and np.array_equal(out, stored[ok][order])
        same = np.nonzero(np.diff(vs.astype(np.float64)) == 0)[0]
        assert same.size >= 19 and np.all(order[same] < order[same + 1]), "equal v: the earlier row stays ahead"
    # with audio: sorted by the final v
    audio = feats[5]
    v, _ = eo.values(wide, user, eo.COSINE, 0.25, 1.0, feats, audio)
    out, vs, fs = sc.rising(stored, v, feats)
    wide_out = out if storage == "f32" else widen(out, storage)
    again, _ = eo.values(wide_out, user, eo.COSINE, 0.25, 1.0, fs, audio)
    assert np.array_equal(eo.bits(again), eo.bits(vs)) and np.all(np.diff(again[np.isfinite(again)].astype(np.float64)) >= 0)
    assert ec.same_floats(eo.values(wide_out, user, eo.COSINE, -0.25, -1.0, fs, audio)[0], -again)


def test_holes_have_no_key_under_dot():
    n, d, tile, grid = sc.sizes(64, 4, 3), 128, 64, 4
    mask = sc.holes(n, tile, grid, [64, 63, 10])
    rows = np.random.default_rng(1).standard_normal((n, d), dtype=F32)
    table = sc.with_holes(rows, mask, F32(np.nan))
    v, _ = eo.values(table, rows[0], eo.DOT, 1.0)
    assert np.array_equal(np.isnan(v), mask) and np.array_equal(table[~mask], rows[: int((~mask).sum())])
    assert sc.finite_counts(v, tile, grid)[:, :3].tolist() == [[64, 63, 10]] * 4
    from spotify_recommender_amd.embed_half import widen
    for storage, word in sc.NAN_WORD.items():
        assert np.isnan(widen(np.array([word], np.uint16), storage)[0])


def test_plateau_is_the_top_and_its_lowest_rows_are_the_answer():
    n, d = 6001, 16
    table, default, flat = sc.plateau(n, d, max_run=50)
    assert int(flat.sum()) == int(0.4 * n) and np.all(table[flat] == default)
    runs = np.diff(np.nonzero(np.diff(np.concatenate([[0], flat.view(np.int8), [0]])))[0])[::2]
    assert runs.size > 20 and runs.min() >= 1   # (runs that land side by side merge: no upper bound)
    v, _ = eo.values(table, default, eo.COSINE, 1.0)
    assert np.all(v[flat] == v.max()) and np.all(v[~flat] < v.max())
    assert np.all(np.diff(v[~flat].astype(np.float64)) >= 0)
    for topn in (10, 128, 1024):
        ids, scores = eo.topn(v, topn)
        assert ids.tolist() == np.nonzero(flat)[0][:topn].tolist() and np.all(scores == v.max())
    gone = np.nonzero(flat)[0][:300].tolist()
    assert eo.topn(v, 10, gone)[0].tolist() == np.nonzero(flat)[0][300:310].tolist()


def test_the_quick_topn_is_the_oracle_s():
    rng = np.random.default_rng(4)
    v = rng.standard_normal(5000).astype(F32)
    v[100:900] = v[7]                      # a plateau across the cut
    v[[3, 4000]] = np.nan
    v[[5, 6]] = [np.inf, -np.inf]
    v[[10, 11]] = [0.0, -0.0]
    for base in (0, 1_000_000):
        for topn in (1, 10, 257, 1024, 4990, 6000):
            for excl in ((), [base + 100, base + 101, 7, base + 4999, base + 9999, -3]):
                a, b = eo.topn(v, topn, excl, base), sc.topn(v, topn, excl, base)
                assert a[0].tolist() == b[0].tolist() and np.array_equal(eo.bits(a[1]), eo.bits(b[1])), (base, topn, excl)
    for vv in (-v, np.zeros(300, F32), np.full(5, np.nan, F32)):
        a, b = eo.topn(vv, 128), sc.topn(vv, 128)
        assert a[0].tolist() == b[0].tolist() and np.array_equal(eo.bits(a[1]), eo.bits(b[1]))


# ---- the cases themselves, against the CPU placement of the fp32 library ----------------------------------------------------

def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU placement is never taken here")


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


@cpu_only
@pytest.mark.parametrize("what", ["cosine", "dot", "audio"])
@pytest.mark.parametrize("d", sc.DIMS)
def test_rising_and_falling_tables_on_the_cpu_placement(engine_lib, d, what):
    from spotify_recommender_amd.embed import EmbeddingTable
    n = 4099
    rng = np.random.default_rng(d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    req = dict(sc.SINGLE_REQUESTS[what], user=rng.standard_normal(d, dtype=F32))
    if what == "audio":
        req["audio"] = rng.random(12, dtype=F32)
    v = ec.expected(feats, table, req)[0]
    table, v, feats = sc.rising(table, v, feats)
    falling = dict(req, embed_weight=-req["embed_weight"])
    if what == "audio":
        falling["audio_weight"] = -req["audio_weight"]
    with _node(feats) as nd, EmbeddingTable(nd, table) as tab:
        ec.check(tab, feats, table, req, f"rising {what} d={d}")
        assert set(tab.query(**req)[0].tolist()) <= set(range(n - 1 - 2 * req["topn"], n)), "the answer of a rising table is its end"
        ec.check(tab, feats, table, falling, f"falling {what} d={d}")
        ec.check(tab, feats, table, dict(req, exclude=list(range(n - 40, n, 3))), f"rising {what} d={d}, best rows excluded")
        ec.check(tab, feats, table, dict(falling, exclude=list(range(0, 40, 3))), f"falling {what} d={d}, best rows excluded")


@cpu_only
@pytest.mark.parametrize("d", [16, 64])
def test_the_plateau_on_the_cpu_placement(engine_lib, d):
    from spotify_recommender_amd.embed import EmbeddingTable
    n = 6001
    table, default, flat = sc.plateau(n, d, max_run=50)
    feats = np.random.default_rng(d).random((n, 12), dtype=F32)
    first = np.nonzero(flat)[0]
    with _node(feats) as nd, EmbeddingTable(nd, table) as tab:
        for topn in (10, 128, 1024):
            req = dict(user=default, metric="cosine", embed_weight=1.0, topn=topn)
            ec.check(tab, feats, table, req, f"plateau d={d} top-{topn}")
            assert tab.query(**req)[0].tolist() == first[:topn].tolist()
        req = dict(user=default, metric="cosine", embed_weight=1.0, topn=128, exclude=first[:300].tolist())
        ec.check(tab, feats, table, req, f"plateau d={d}, 300 plateau rows excluded")
        assert tab.query(**req)[0].tolist() == first[300:428].tolist()
