"""The embedding scans' STEADY STATE on the GPU (csrc/embed.hip.h's embed_scan_body under the fp32 and the half layouts,
csrc/embed_batch.hip.h), bit for bit against tests/embed_oracle.py: tables large enough that EVERY workgroup of the shipped
grid scans four tiles or more (64 MiB and up; tests/embed_steady_cases.py has the sizes and the list-occupancy model), so
the tile loop's carry — cur_e, the audio vector cur_s, the threshold in registers — repeated mid-loop compaction and the
hand-back of a new threshold are exercised at every dim of all three libraries.  RISING tables (v non-decreasing in the row
index: every row of every round is appended) and the same tables FALLING (negated weights: the answer lies in round 0);
the BOUND cases, whose lists are written up to their last slot; one MIXED batch pass; PLATEAUS of 40 % equal scores; the
batch library against the single-user one.  Each test asserts the grid and the rounds it relies on, so another grid rule
fails here instead of testing nothing."""
import functools

import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_half_cases as hc
from tests import embed_oracle as eo
from tests import embed_steady_cases as sc

pytestmark = pytest.mark.gpu
F32 = np.float32
HALF = ("fp16", "bf16")


@functools.lru_cache(maxsize=None)
def _grid():
    """min(2 * compute units, the merge's lists): what embed_grid gives a table of at least that many tiles."""
    from spotify_recommender_amd import CosineEngine
    with CosineEngine(np.ones((1, 12), F32)) as eng:
        return sc.grid_of(eng.stats().compute_units)


def _open(kind, feats, stored):
    from spotify_recommender_amd import CosineEngine
    eng = CosineEngine(feats)
    if kind == "batch":
        from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
        return eng, EmbeddingBatchTable(eng, stored)
    if kind in HALF:
        from spotify_recommender_amd.embed_half import HalfEmbeddingTable
        return eng, HalfEmbeddingTable(eng, hc.as_given(stored, kind))
    from spotify_recommender_amd.embed import EmbeddingTable
    return eng, EmbeddingTable(eng, stored)


def _stored(kind, table):
    """(what the library is given, the float32 table the contract speaks of)."""
    if kind in HALF:
        from spotify_recommender_amd.embed_half import to_storage, widen
        words = to_storage(table, kind)
        return words, widen(words, kind)
    return table, table


def _widened(kind, stored):
    if kind in HALF:
        from spotify_recommender_amd.embed_half import widen
        return widen(stored, kind)
    return stored


def _steady(tab, layout, n, rounds):
    """The state the test is about, asked of the library."""
    info = tab.info()
    assert info["grid"] == _grid() and info["tile_rows"] == layout.tile_rows and info["rows"] == n, info
    assert -(-n // layout.tile_rows) >= rounds * _grid()


# ---- rising and falling ---------------------------------------------------------------------------------------------------------

def _values(wide, feats, req):
    """(v, c) of every row of a single-user request by the oracle."""
    return eo.values(wide, req["user"], eo.DOT if req["metric"] == "dot" else eo.COSINE, req["embed_weight"], req.get("audio_weight", 0.0),
                     feats, req.get("audio"))


@functools.lru_cache(maxsize=1)
def _rising_table(kind, d, what, rounds):
    """(feats, stored table, request, v of every row): random rows sorted by the oracle's v of the request.  v is a
    function of the row alone, so the sorted v IS the oracle's v of the sorted table (tests/test_embed_steady_cpu.py)."""
    layout = sc.Layout(kind, d)
    n = sc.sizes(layout.tile_rows, _grid(), rounds)
    rng = np.random.default_rng(7000 * d + rounds + len(what))
    feats = rng.random((n, 12), dtype=F32)
    stored, wide = _stored(kind, rng.standard_normal((n, d), dtype=F32))
    user = rng.standard_normal(d, dtype=F32)
    if what in sc.SINGLE_REQUESTS:
        req = dict(sc.SINGLE_REQUESTS[what], user=user)
    else:
        req = dict(metric=what, embed_weight=1.0, user=user)
    if what == "audio":
        req["audio"] = rng.random(12, dtype=F32)
    v, _ = _values(wide, feats, req)
    del wide
    stored, v, feats = sc.rising(stored, v, feats)
    return feats, stored, req, v


SINGLE_RISING = [c for c in sc.rising_cases() if c[0] != "batch"]


@pytest.mark.parametrize("kind,d,what,topns", SINGLE_RISING, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in SINGLE_RISING])
def test_rising_and_falling_tables(kind, d, what, topns):
    """cosine top-10, dot top-257 and (d = 32, 128) a request with audio, each on a table sorted by ITS v; the falling
    variant negates every weight, which negates every v exactly."""
    layout = sc.Layout(kind, d)
    rounds = sc.rising_rounds(kind, d, topns)
    feats, stored, req, v = _rising_table(kind, d, what, rounds)
    n = v.size
    peak, compactions, room = sc.peaks(layout, v, _grid(), req["topn"])
    assert compactions >= 2 and peak <= layout.capacity and room <= layout.capacity
    falling = dict(req, embed_weight=-req["embed_weight"])
    if "audio_weight" in req:
        falling["audio_weight"] = -req["audio_weight"]
    eng, tab = _open(kind, feats, stored)
    with eng, tab:
        _steady(tab, layout, n, rounds)
        gi, _ = sc.check_query(tab, req, v, f"rising {kind} d={d} {what}")
        assert gi.min() >= n - 2 * req["topn"] - 1, "the answer of a rising table is its end"
        sc.check_query(tab, falling, -v, f"falling {kind} d={d} {what}")
        # The answer of a rising table lies in its last tiles (of a falling one in its first).  A second, unrelated user on
        # the same table has its answer spread over every round, and the parity hook states v and c of every row of every
        # tile: a value that goes wrong in a middle round shows here.
        other = dict(req, user=np.random.default_rng(d).standard_normal(d, dtype=F32), topn=257)
        ov, oc = _values(_widened(kind, stored), feats, other)
        sc.check_query(tab, other, ov, f"another user, {kind} d={d} {what}")
        gv, gc = tab.scores(**{k: x for k, x in other.items() if k != "topn"})
        assert ec.same_floats(gc, oc), f"{kind} d={d} {what}: c differs in {int(np.sum(eo.bits(gc) != eo.bits(oc)))} rows"
        assert ec.same_floats(gv, ov), f"{kind} d={d} {what}: v differs in {int(np.sum(eo.bits(gv) != eo.bits(ov)))} rows"
        if d in (32, 128):   # some of the best rows of either direction are excluded
            excl = list(range(n - 60, n, 3)) + list(range(0, 60, 3)) + [n - 1, n + 7]
            sc.check_query(tab, dict(req, exclude=excl), v, f"rising {kind} d={d} {what}, exclusions")
            sc.check_query(tab, dict(falling, exclude=excl), -v, f"falling {kind} d={d} {what}, exclusions")


def _user_values(table, us, metric, w=1.0):
    return [eo.values(table, u, eo.DOT if metric == "dot" else eo.COSINE, w)[0] for u in us]


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("d", sc.DIMS)
def test_rising_and_falling_tables_in_batches(d, metric):
    """Eight users that are exact multiples of one vector: one order for all, so all eight lists fill, compact and take
    their new thresholds in the same tiles; top-1, 10 and 128, rising and falling."""
    layout = sc.Layout("batch", d)
    rounds = sc.rising_rounds("batch", d, sc.BATCH_TOPNS)
    feats, table, req, v = _rising_table("batch", d, metric, rounds)
    n = v.size
    for topn in sc.BATCH_TOPNS:
        peak, compactions, _ = sc.peaks(layout, v, _grid(), topn)
        assert compactions >= 2 and peak <= layout.capacity
    us = np.stack([F32(p) * req["user"] for p in sc.POWERS])
    vs = _user_values(table, us, metric)
    assert all(np.all(np.diff(x.astype(np.float64)) >= 0) for x in vs), "a power of two scales exactly: every user rises"
    eng, tab = _open("batch", feats, table)
    with eng, tab:
        _steady(tab, layout, n, rounds)
        assert tab.info()["pass_users"] == len(us)
        for topn in sc.BATCH_TOPNS:
            sc.check_users(tab, us, vs, n_top=topn, metric=metric, embed_weight=1.0, what=f"rising d={d}")
            sc.check_users(tab, us, [-x for x in vs], n_top=topn, metric=metric, embed_weight=-1.0, what=f"falling d={d}")


# ---- the bound cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,d,topn,per_round,rounds,short", sc.BOUND_CASES, ids=[f"{c[0]}-{c[1]}" for c in sc.BOUND_CASES])
def test_a_list_is_filled_to_its_last_slot(kind, d, topn, per_round, rounds, short):
    """metric="dot", a rising table whose holes (rows with a NaN: no key) leave exactly `per_round` appends per workgroup
    and round: the model's peak is the list's capacity (batch) or one less (single), never more — asserted before launch."""
    layout = sc.Layout(kind, d)
    grid = _grid()
    n = sc.sizes(layout.tile_rows, grid, rounds)
    mask = sc.holes(n, layout.tile_rows, grid, per_round)
    rng = np.random.default_rng(900 * d + rounds)
    feats = rng.random((n, 12), dtype=F32)
    user = rng.standard_normal(d, dtype=F32)
    stored, wide = _stored(kind, rng.standard_normal((int((~mask).sum()), d), dtype=F32))
    stored, _, _ = sc.rising(stored, eo.values(wide, user, eo.DOT, 1.0)[0])
    stored = sc.with_holes(stored, mask, sc.NAN_WORD[kind] if kind in HALF else F32(np.nan))
    wide = _widened(kind, stored)
    us = np.stack([F32(p) * user for p in sc.POWERS]) if kind == "batch" else user[None]
    vs = _user_values(wide, us, "dot")
    for v in vs:
        assert np.array_equal(np.isnan(v), mask) and np.all(np.diff(v[~mask].astype(np.float64)) >= 0)
        peak, _, room = sc.peaks(layout, v, grid, topn)
        assert peak == layout.capacity - short and room <= layout.capacity, "the case is not the one the model was run on"
    eng, tab = _open(kind, feats, stored)
    with eng, tab:
        _steady(tab, layout, n, rounds)
        if kind == "batch":
            sc.check_users(tab, us, vs, n_top=topn, metric="dot", embed_weight=1.0, what=f"bound d={d}")
        else:
            sc.check_query(tab, dict(user=user, metric="dot", embed_weight=1.0, topn=topn), vs[0], f"bound {kind}")
            sc.check_query(tab, dict(user=user, metric="dot", embed_weight=-1.0, topn=topn), -vs[0], f"bound {kind}, falling")


# ---- one mixed pass, and the batch against the single call -----------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("d", sc.DIMS)
def test_one_mixed_pass_in_the_steady_state(d, metric):
    """Four rising users, one that falls, a random one, the zero vector (every v is 0: a plateau over the whole table) and
    one that excludes the best 1000 rows, in one pass; and what each gets alone."""
    layout = sc.Layout("batch", d)
    rounds = sc.rising_rounds("batch", d, sc.BATCH_TOPNS)
    feats, table, req, v = _rising_table("batch", d, metric, rounds)
    n, u = v.size, req["user"]
    rng = np.random.default_rng(d)
    us = np.stack([u, F32(2) * u, F32(0.5) * u, F32(4) * u, -u, rng.standard_normal(d, dtype=F32), np.zeros(d, F32), u])
    lists = [[] for _ in us]
    lists[7] = list(range(n - 1000, n))
    vs = _user_values(table, us, metric)
    assert np.all(vs[6] == 0)
    eng, tab = _open("batch", feats, table)
    with eng, tab:
        _steady(tab, layout, n, rounds)
        ids, scores, counts = sc.check_users(tab, us, vs, n_top=128, metric=metric, embed_weight=1.0, exclude=lists, what=f"mixed d={d} {metric}")
        assert ids[6].tolist() == list(range(128)) and ids[7].max() == n - 1001 and ids[4].max() < 3 * 128
        for b in range(len(us)):
            ai, asc, ac = tab.query_users(users=us[b : b + 1], topn=128, metric=metric, embed_weight=1.0, exclude=[lists[b]])
            assert ai[0].tolist() == ids[b].tolist() and np.array_equal(eo.bits(asc[0]), eo.bits(scores[b])) and ac[0] == counts[b], b


def test_the_batch_equals_the_single_call_on_a_rising_table():
    from spotify_recommender_amd.embed import EmbeddingTable
    d = 64
    layout = sc.Layout("batch", d)
    rounds = sc.rising_rounds("batch", d, sc.BATCH_TOPNS)
    feats, table, req, v = _rising_table("batch", d, "cosine", rounds)
    u = req["user"]
    us = np.stack([F32(p) * u for p in sc.POWERS] + [-u, np.zeros(d, F32), np.random.default_rng(1).standard_normal(d, dtype=F32)])
    eng, tab = _open("batch", feats, table)
    with eng, tab, EmbeddingTable(eng, table) as single:
        _steady(tab, layout, v.size, rounds)
        _steady(single, sc.Layout("f32", d), v.size, rounds)
        for metric, w, topn in (("cosine", 1.0, 128), ("dot", 1.0, 10), ("cosine", -1.0, 1)):
            ids, scores, counts = tab.query_users(users=us, topn=topn, metric=metric, embed_weight=w)
            for b in range(len(us)):
                si, ss = single.query(user=us[b], metric=metric, embed_weight=w, topn=topn)
                assert counts[b] == si.size == topn and ids[b].tolist() == si.tolist(), (metric, b)
                assert np.array_equal(eo.bits(scores[b]), eo.bits(ss)), (metric, b)


# ---- plateaus ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("kind", sc.KINDS)
def test_a_plateau_of_equal_scores_is_cut_at_the_lowest_rows(kind, d):
    """40 % of the rows are one default vector, in runs of 1 to 5000, and the user is that vector: the plateau is the top
    and the row index alone decides; three rounds."""
    layout = sc.Layout(kind, d)
    rounds = 3
    n = sc.sizes(layout.tile_rows, _grid(), rounds)
    table, default, flat = sc.plateau(n, d)
    stored, wide = _stored(kind, table)
    user = wide[np.argmax(flat)].copy()
    feats = np.random.default_rng(d).random((n, 12), dtype=F32)
    first = np.nonzero(flat)[0]
    assert first.size >= 1024 + 300, "the plateau is deeper than any answer asked for"
    gone = first[:300].tolist()
    us = np.stack([F32(p) * user for p in sc.POWERS]) if kind == "batch" else user[None]
    vs = _user_values(wide, us, "cosine")
    for v in vs:
        assert np.all(v[flat] == v.max()) and np.all(v[~flat] < v.max())
    eng, tab = _open(kind, feats, stored)
    with eng, tab:
        _steady(tab, layout, n, rounds)
        for topn in (10, 128, 1024):
            if topn > layout.max_topn:
                continue
            if kind == "batch":
                ids, _, _ = sc.check_users(tab, us, vs, n_top=topn, metric="cosine", embed_weight=1.0, what=f"plateau d={d}")
                assert all(row.tolist() == first[:topn].tolist() for row in ids)
            else:
                gi, _ = sc.check_query(tab, dict(user=user, metric="cosine", embed_weight=1.0, topn=topn), vs[0], f"plateau {kind} d={d} top-{topn}")
                assert gi.tolist() == first[:topn].tolist()
        if kind == "batch":
            ids, _, _ = sc.check_users(tab, us, vs, n_top=128, metric="cosine", embed_weight=1.0, exclude=[gone] * len(us), what=f"plateau d={d}, excluded")
            assert all(row.tolist() == first[300:428].tolist() for row in ids)
        else:
            gi, _ = sc.check_query(tab, dict(user=user, metric="cosine", embed_weight=1.0, topn=128, exclude=gone), vs[0], f"plateau {kind} d={d}, excluded")
            assert gi.tolist() == first[300:428].tolist()
