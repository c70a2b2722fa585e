"""The candidate gather's STEADY STATE on the GPU (csrc/embed_cand.hip.h's embed_cand_kernel, selecting and scoring form),
bit for bit and with a leave-out budget of 0 cases: lists that feed ONE workgroup several full rounds of rows that all beat
its threshold (tests/embed_cand_steady_cases.py has the lists and the list-occupancy model), so the loop's three-deep carry
(cur_r / next_r / far_r, cur_e, the audio values cur_s), its mid-loop compaction and threshold, its LDS exclusion search with
a threshold standing and the clearing of EVERY owner's claim word — a rejected row's too — are held to tests/embed_oracle.py
over the listed rows, to RestrictedEmbeddingTable.query(only=rowset(ids)) and to the synchronous libraries' scores.  RISING
lists and the same lists FALLING (every weight negated), the FULLEST lists (kCandLimit - 1 keys and a full tile on top), a
PLATEAU fed in falling id order, every row listed TWICE, a row base.  Every table has 4096 rows.  Each test asserts the
grid, the tile size and the list's tile count it relies on, and runs the model on its own list before it launches: another
grid or trigger rule fails here instead of testing nothing."""
import functools

import numpy as np
import pytest

from tests import embed_cand_steady_cases as cs
from tests import embed_cases as ec
from tests.test_gpu_embed_cand import _check_rank, _check_scores, _dev, _Opened, _oracle_rank, _rank, _same, _sync_scores

pytestmark = pytest.mark.gpu
F32 = np.float32


def _list(ids):
    """A case's list is shared between tests and read-only; torch is handed a copy it may call writable."""
    return np.array(ids, np.int64)


@functools.lru_cache(maxsize=None)
def _compute_units():
    from spotify_recommender_amd import CosineEngine
    with CosineEngine(np.ones((1, 12), F32)) as eng:
        return int(eng.stats().compute_units)


def _open(o):
    return _Opened(o.feats, o.wide, o.storage, **({"row_base": o.row_base} if o.row_base else {}))


def _steady(op, o, ids, topns, twice=True):
    """The state the test is about, asked of the library and of the model before anything is launched."""
    info = op.ct.info()
    assert 2 * _compute_units() >= o.G, f"a device of {_compute_units()} compute units runs no grid of {o.G}"
    assert (info["grid"], info["tile_rows"], info["rows"], info["dim"]) == (o.G, o.t, o.n, o.d), info
    assert cs.table_grid(o.n, o.t, _compute_units()) == o.G and ec.same_floats(op.wide, o.wide)
    tiles, grid = cs.list_shape(o, ids)
    assert grid == o.G and tiles == o.rounds * o.G + o.b + 1, "workgroup b's rounds are tiles b, b + G, ..."
    for topn in topns if twice else ():
        got = cs.model(o, ids, topn)
        assert got["compactions"] >= 2 and got["peak"] <= o.layout.capacity and got["sort_room"] <= o.layout.capacity, (topn, got)


def _rank_kw(req):
    return {k: x for k, x in req.items() if k not in ("user", "exclude")}


def _again_and_every_row(op, o, v, ids, req, what):
    """The same rank call twice with no synchronise between them, then — still without one — a top-1024 dot call over every
    1024 rows of the table: both answers are the oracle's, and every finite row of the table is returned (a claim left
    standing, by a row the threshold rejected for one, would make the next call drop that row)."""
    import torch
    user, dev_ids = _dev(np.asarray(req["user"], F32)), _dev(np.asarray(ids, np.int64))
    excl = _dev(np.asarray(req["exclude"], np.int64)) if req.get("exclude") else None
    pair = [op.ct.rank(user, dev_ids, exclude=excl, **_rank_kw(req)) for _ in range(2)]
    chunks = [np.arange(lo, min(lo + 1024, o.n), dtype=np.int64) + o.row_base for lo in range(0, o.n, 1024)]
    dev_chunks = [_dev(c) for c in chunks]
    swept = [op.ct.rank(user, c, topn=1024, metric="dot", embed_weight=1.0) for c in dev_chunks]
    torch.cuda.current_stream().synchronize()
    want = _oracle_rank(op, v, ids, req)
    for i, (idx, sc, cnt) in enumerate(pair):
        _same((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())), want, req["topn"], f"{what}, call {i + 1} of two back to back")
    dot = cs._values(o.wide, o.feats, dict(user=req["user"], metric="dot", embed_weight=1.0))
    for c, (idx, sc, cnt) in zip(chunks, swept):
        got = (idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item()))
        rows = c - o.row_base
        assert got[2] == int(np.isfinite(dot[rows]).sum()), f"{what}: a call over rows {rows[0]}.. returned {got[2]} of them: a claim was left behind"
        _same(got, _oracle_rank(op, dot, c, dict(topn=1024)), 1024, f"{what}, then every row from {rows[0]} on")


def _scores(op, o, v, ids, req, what):
    """v, c and the flag of every entry in list order against the synchronous library, which is the oracle's."""
    sv, sc = _sync_scores(op, req)
    wv, wc, _, _ = ec.expected(o.feats, o.wide, dict(req, topn=1, exclude=[]))
    assert ec.same_floats(wv, v) and ec.same_floats(sv, wv) and ec.same_floats(sc, wc), f"{what}: the synchronous library differs from the oracle"
    _check_scores(op, sv, sc, ids, req, what)


def _held(op, o, ids, req, what, exclusions=True):
    """One list under one request: rank, rank again, every row, scores, and the two exclusion lists."""
    v = cs._values(o.wide, o.feats, req)
    got = _check_rank(op, v, ids, req, what)
    _again_and_every_row(op, o, v, ids, req, what)
    _scores(op, o, v, ids, req, what)
    if exclusions:
        excl, _ = cs.exclusions(o, req, ids)
        left = _check_rank(op, v, ids, dict(req, exclude=excl), f"{what}, 1024 exclusions")
        assert left[0][: left[2]].tolist() != got[0][: got[2]].tolist(), "the list excludes rows of the answer"
        _again_and_every_row(op, o, v, ids, dict(req, exclude=excl), f"{what}, 1024 exclusions")
        best = int(got[0][0])
        one = _check_rank(op, v, ids, dict(req, exclude=[best]), f"{what}, the best row excluded")
        assert best not in one[0].tolist() and one[0][0] == got[0][1]
    return got


@pytest.mark.parametrize("case", cs.RISING, ids=cs.case_id)
def test_rising_and_falling_lists(case):
    """cosine top-10, dot top-257 and (d = 32, 128) a request with audio, each over a table sorted by ITS v: workgroup b is
    fed the best rows, rising; the falling variant negates every weight, over the same list and over the list that holds
    workgroup b's rows alone (its round 0 is the answer, its threshold shuts out every later round)."""
    o = cs.build(case)
    ids, ids_alone = _list(o.ids), _list(o.ids_alone)
    mine = np.concatenate(o.rounds_rows)
    what = cs.case_id(case)
    with _open(o) as op:
        _steady(op, o, ids, o.topns)
        _steady(op, o, ids_alone, o.topns)
        got = _held(op, o, ids, o.req, f"rising {what}")
        assert set(got[0].tolist()) <= set(mine[-(2 * o.req["topn"] + 1):].tolist()), "the answer of a rising list is workgroup b's end"
        falling = cs.negated(o.req)
        _held(op, o, ids, falling, f"falling {what}")
        alone = _held(op, o, ids_alone, falling, f"falling {what}, workgroup {o.b} alone")
        assert alone[0].tolist() == mine[: o.req["topn"]].tolist(), "the answer is the head of workgroup b's list (top-10: of its round 0)"
        # an unrelated user on the rising list: its answer is spread over every round of every workgroup
        other = dict(o.req, user=np.random.default_rng(o.d).standard_normal(o.d, dtype=F32), topn=257)
        _held(op, o, ids, other, f"another user, {what}", exclusions=False)


def test_a_rising_list_over_a_row_base():
    """Ids, exclusions and answers are global; a local row number offered as an exclusion excludes nothing."""
    base = 1_000_000
    o = cs.build(cs.BASED, base)
    ids = _list(o.ids)
    mine = np.concatenate(o.rounds_rows)
    with _open(o) as op:
        _steady(op, o, ids, o.topns)
        for name, req in (("rising", o.req), ("falling", cs.negated(o.req))):
            got = _held(op, o, ids, req, f"row_base {name}")
            assert got[2] == req["topn"] and got[0].min() >= base
            v = cs._values(o.wide, o.feats, req)
            local = [int(x) - base for x in got[0]]   # the answer's LOCAL row numbers: no id of this shard
            same = _check_rank(op, v, ids, dict(req, exclude=local), f"row_base {name}, local rows as exclusions")
            assert same[0].tolist() == got[0].tolist()
        assert set((got[0] - base).tolist()).isdisjoint(mine.tolist()), "the falling answer lies outside workgroup b"
        assert _rank(op, ids - base, o.req)[2] == 0, "local rows are not ids"


@pytest.mark.parametrize("case", cs.FULLEST, ids=cs.case_id)
def test_a_list_enters_a_tile_one_key_short_of_its_limit(case):
    """Top-1024 under dot: workgroup b holds kCandLimit - 1 keys when it enters a full tile, so the model's peak is
    kCandLimit - 1 + t (at d = 16 the list's last slot but one), asserted before launch.  The short entry is a -1, or a row
    with a NaN: claimed, scored and cleared, and no key."""
    o = cs.build(case)
    ids, ids_alone = _list(o.ids), _list(o.ids_alone)
    L = o.layout.k["kCandLimit"]
    what = cs.case_id(case)
    with _open(o) as op:
        _steady(op, o, ids, [1024])
        assert cs.model(o)["peak"] == L - 1 + o.t, "the case is not the one the model was run on"
        if o.d == 16:
            assert cs.model(o)["peak"] == o.layout.capacity - 1
        got = _held(op, o, ids, o.req, what, exclusions=False)
        assert got[2] == 1024
        if o.nan_row is not None:
            assert np.isnan(o.v[o.nan_row]) and o.nan_row not in got[0].tolist()
            op.ct.rank(_dev(o.req["user"]), _dev(ids), topn=1024, metric="dot", embed_weight=1.0)   # (the call directly in front claims the row)
            cosine = dict(user=o.req["user"], metric="cosine", embed_weight=1.0, topn=10)
            few = np.array([o.nan_row, 0, 1], np.int64)
            seen = _check_rank(op, cs._values(o.wide, o.feats, cosine), few, cosine, f"{what}: the NaN row under cosine")
            assert seen[2] == 3 and o.nan_row in seen[0].tolist(), "its claim was cleared although it formed no key"
        _held(op, o, ids, cs.negated(o.req), f"{what}, falling", exclusions=False)


@pytest.mark.parametrize("case", cs.PLATEAU, ids=cs.case_id)
def test_a_plateau_in_falling_id_order(case):
    """40 % of the table is one vector and the user is that vector.  Workgroup b is fed rising rows up to its first
    compaction at top-1024 and then the whole plateau by falling id: every later row is a better key at an equal v, so every
    row of every round is appended and the answer — the lowest plateau ids — arrives last."""
    o = cs.build(case)
    ids, ids_alone = _list(o.ids), _list(o.ids_alone)
    what = cs.case_id(case)
    with _open(o) as op:
        _steady(op, o, ids, o.topns)
        for topn in o.topns:
            req = dict(o.req, topn=topn)
            got = _held(op, o, ids, req, f"{what} top-{topn}", exclusions=topn == 128)
            assert got[0].tolist() == o.plateau[:topn].tolist()
        gone = [int(x) for x in o.plateau[:300]]
        left = _check_rank(op, o.v, ids, dict(o.req, topn=128, exclude=gone), f"{what}, the lowest 300 excluded")
        assert left[0].tolist() == o.plateau[300:428].tolist()


@pytest.mark.parametrize("case", cs.TWICE, ids=cs.case_id)
def test_every_row_listed_twice(case):
    """A rising list whose rows are each listed a second time in the tiles of other workgroups: which copy wins the claim
    varies from run to run, the answer does not, and the count is that of the distinct rows."""
    o = cs.build(case)
    ids, ids_alone = _list(o.ids), _list(o.ids_alone)
    mine = np.concatenate(o.rounds_rows)
    what = cs.case_id(case)
    with _open(o) as op:
        _steady(op, o, ids, o.topns, twice=False)
        _steady(op, o, ids_alone, o.topns)
        for i in range(3):
            got = _held(op, o, ids, o.req, f"{what}, run {i}", exclusions=i == 0)
            assert np.unique(got[0]).size == got[2] == o.req["topn"]
            assert set(got[0].tolist()) <= set(mine[-(2 * o.req["topn"] + 1):].tolist())
        few = np.concatenate([mine[:400], [-1], mine[:400][::-1], mine[200:300]])
        req = dict(o.req, topn=1024)
        short = _check_rank(op, o.v, few, req, f"{what}: 400 rows in 900 entries")
        assert short[2] == 400
        _scores(op, o, o.v, few, o.req, f"{what}: 400 rows in 900 entries")
