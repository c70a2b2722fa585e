"""The result path of the synchronous host API (csrc/engine_sync.hip.h: sync_begin / sync_finish) on the MI355X, at its own
boundaries: results whose last launch raises the completion word (one round, topn <= 1024), results stored straight into
pinned host memory (<= 2048 slots), results copied back (more), all rows, and a caller's buffer longer than the rows can
fill.  One handle of 4 100 seeded random rows (no ties at this size); every call through the C-ABI with raw buffers, compared
bit for bit with the oracle: ids, score bits, the count, and -1 / +0.0f behind it up to topn.  Then the same calls again
interleaved on the same handle and on a fresh one, so that the slot buffers regrow between calls and a notifying call
follows one that waited for the stream."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import expected_from_scores as expected_labels
from tests.playlist_labels_oracle import expected_diverse, expected_scored, scores_of
from tests.prior_oracle import request_call

pytestmark = pytest.mark.gpu

N = 4100
TOPNS = (1, 1024, 1025, 2048, 2049, 4100, 5000)   # the notify limit, the direct limit, all rows, padding
Q_ROW = 17                                        # the query row (label 2) ...
Q_VEC_EXCLUDE = 3000                              # ... and the row a query by value excludes
BIG_LABEL, BIG_LABEL_ROWS = 0, 2049               # one label holds one row more than the pinned slots
SMALL_LABEL, SMALL_LABEL_ROWS = 1, 30
MEMBERS = [5, 1234, 4099]
LAM, CAP = 0.7, 2


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _raw(fn, h, head, tail, topn, batch=1):
    """fn(h, *head, topn, idx, score, counts) on buffers full of garbage: (idx, score, counts) as the call left them."""
    idx = np.full((batch, topn), -7, np.int64)
    score = np.full((batch, topn), 9.0, np.float32)
    counts = np.full(batch, -7, np.int32)
    rc = fn(h, *head, *tail, int(topn), _ptr(idx), _ptr(score), counts.ctypes.data_as(fn.argtypes[-1]))
    assert rc == 0, rc
    return idx, score, counts


def _same(got, want, topn, what):
    """One query's row of _raw against (ids, scores) of the oracle: ids, score bits, the count and the padding."""
    idx, score, count = got
    wi, ws = want
    c = len(wi)
    assert c <= topn and count == c, f"{what}: count {count}, expected {c}"
    assert idx[:c].tolist() == np.asarray(wi).tolist(), f"{what}: ids differ"
    assert np.array_equal(score[:c].view(np.uint32), (np.asarray(ws, np.float32) + np.float32(0)).view(np.uint32)), f"{what}: scores differ"
    assert np.all(idx[c:] == -1), f"{what}: ids behind the count are not -1"
    assert not score[c:].view(np.uint32).any(), f"{what}: scores behind the count are not +0.0f"


def _same3(got, want, what, pool_rows=None):
    """A request_call result (it has checked the padding itself) against (ids, rel[, mmr]) of the oracle."""
    rc, ids, sc, mmr, p = got
    assert rc == 0, f"{what}: rc {rc}"
    assert ids.tolist() == np.asarray(want[0]).tolist(), f"{what}: ids differ"
    assert np.array_equal(sc.view(np.uint32), (np.asarray(want[1], np.float32) + np.float32(0)).view(np.uint32)), f"{what}: scores differ"
    if len(want) > 2:
        assert np.array_equal(mmr.view(np.uint32), np.asarray(want[2], np.float32).view(np.uint32)), f"{what}: mmr differs"
    if pool_rows is not None:
        assert p == pool_rows, f"{what}: pool_rows {p}, expected {pool_rows}"


@pytest.fixture(scope="module")
def world(engine_lib):
    """The catalogue, its side data and every expected answer, computed once and never modified:
    (feats, labels, groups, {case name: (call(engine), check(result))})."""
    from spotify_recommender_amd import capi
    feats = np.ascontiguousarray(oracle.mt19937_uniform(4100, N))
    rng = np.random.default_rng(41)
    labels = np.full(N, 2, np.int32)
    perm = rng.permutation(N)
    perm = perm[~np.isin(perm, [Q_ROW] + MEMBERS)]   # (the query row and the playlist's members keep label 2)
    labels[perm[:BIG_LABEL_ROWS]] = BIG_LABEL
    labels[perm[BIG_LABEL_ROWS:BIG_LABEL_ROWS + SMALL_LABEL_ROWS]] = SMALL_LABEL
    small_rows = np.sort(perm[BIG_LABEL_ROWS:BIG_LABEL_ROWS + SMALL_LABEL_ROWS])
    groups = (np.arange(N) % 7).astype(np.int32)
    lib = capi.lib()
    cases = {}

    s_row = oracle.scores(feats, feats[Q_ROW])
    q_vec = rng.random(12, dtype=np.float32)
    s_vec = oracle.scores(feats, q_vec)
    q_c = np.ascontiguousarray(q_vec)
    for topn in TOPNS:
        cases[f"row top-{topn}"] = (
            lambda e, topn=topn: _raw(lib.mi355rec_query_row_topn, e._h, (Q_ROW,), (), topn),
            lambda got, topn=topn, want=oracle.topn_canonical(s_row, Q_ROW, topn): _same((got[0][0], got[1][0], got[2][0]), want, topn, f"row top-{topn}"))
        cases[f"value top-{topn}"] = (
            lambda e, topn=topn: _raw(lib.mi355rec_query_topn, e._h, (_ptr(q_c), Q_VEC_EXCLUDE), (), topn),
            lambda got, topn=topn, want=oracle.topn_canonical(s_vec, Q_VEC_EXCLUDE, topn): _same((got[0][0], got[1][0], got[2][0]), want, topn, f"value top-{topn}"))

    b_rows = [0, 2050, N - 1]
    b_q = np.ascontiguousarray(feats[b_rows])
    b_ex = np.asarray(b_rows, np.int64)
    b_scores = [oracle.scores(feats, feats[r]) for r in b_rows]
    for topn in (682, 683):   # 3 x 682 = 2046 slots and 3 x 683 = 2049: either side of the direct limit
        def check_batch(got, topn=topn, want=[oracle.topn_canonical(s, r, topn) for s, r in zip(b_scores, b_rows)]):
            for b in range(3):
                _same((got[0][b], got[1][b], got[2][b]), want[b], topn, f"batch of 3 top-{topn}, query {b}")
        cases[f"batch top-{topn}"] = (lambda e, topn=topn: _raw(lib.mi355rec_query_batch_topn, e._h, (_ptr(b_q), 3, _ptr(b_ex)), (), topn, batch=3),
                                      check_batch)

    one_label = np.asarray([BIG_LABEL], np.int32)
    for topn in (2048, 2049, 3000):
        cases[f"label top-{topn}"] = (
            lambda e, topn=topn: _raw(lib.mi355rec_query_row_topn_labels, e._h, (Q_ROW,), (_ptr(one_label), 1), topn),
            lambda got, topn=topn, want=expected_labels(s_row, labels, Q_ROW, [BIG_LABEL], topn): _same((got[0][0], got[1][0], got[2][0]), want, topn, f"label top-{topn}"))

    s_pl = scores_of(feats, feats[MEMBERS])
    top1024 = expected_scored(s_pl, feats, None, None, MEMBERS, 1024)
    request = lib.mi355rec_query_playlist_request
    cases["playlist top-1024"] = (lambda e: request_call(capi, request, e._h, rows=MEMBERS, topn=1024),
                                  lambda got: _same3(got, top1024, "playlist top-1024"))
    # fewer rows left than topn.  (An exclusion list holds at most 1024 ids, so on 4 100 rows it cannot do that alone: a label set
    # of 30 rows, 20 of them excluded.  The scan is asked for min(topn, 30) keys and finds 10.  The exclusion list alone: `tiny`.)
    gone = [int(r) for r in small_rows[:20]]
    few = expected_scored(s_pl, feats, labels, [SMALL_LABEL], MEMBERS + gone, 64)
    assert len(few[0]) == SMALL_LABEL_ROWS - 20
    cases["playlist, 10 rows left for top-64"] = (
        lambda e: request_call(capi, request, e._h, rows=MEMBERS, exclude=gone, labels=[SMALL_LABEL], topn=64),
        lambda got: _same3(got, few, "playlist, 10 rows left for top-64"))
    cases["diverse pool 1024 top-1024"] = (
        lambda e: request_call(capi, request, e._h, rows=MEMBERS, topn=1024, lam=LAM, pool=1024),
        lambda got, want=expected_diverse(top1024, feats, LAM, 1024): _same3(got, want, "diverse pool 1024 top-1024"))
    pool256 = (top1024[0][:256], top1024[1][:256])
    cases["capped pool 256 top-64"] = (
        lambda e: request_call(capi, request, e._h, rows=MEMBERS, topn=64, lam=LAM, pool=256, max_per_group=CAP),
        lambda got, want=expected_diverse(pool256, feats, LAM, 64, groups, CAP): _same3(got, want, "capped pool 256 top-64", pool_rows=256))
    return feats, labels, groups, cases


# small direct call -> 5000 (the slots regrow, no completion word) -> small (a notifying call behind it) -> batch -> label -> playlist
INTERLEAVED = ("row top-1", "row top-5000", "value top-1", "batch top-683", "label top-2049", "playlist top-1024",
               "row top-1024", "value top-5000", "batch top-682", "capped pool 256 top-64", "label top-2048", "row top-1025",
               "diverse pool 1024 top-1024", "value top-2049", "playlist, 10 rows left for top-64", "row top-2048")


def _engine(world):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine
    feats, labels, groups, _ = world
    eng = CosineEngine(feats)
    eng.set_labels(labels)
    eng.set_groups(groups)
    return eng


def _run(eng, cases, names):
    for name in names:
        call, check = cases[name]
        check(call(eng))


def test_every_entry_point_then_interleaved_on_the_same_handle(world):
    cases = world[3]
    assert set(INTERLEAVED) <= set(cases)
    with _engine(world) as eng:
        _run(eng, cases, list(cases))      # ascending sizes per entry point: the slots grow 1024 -> 2048 -> 4096 -> 8192 on the way
        _run(eng, cases, INTERLEAVED)
        _run(eng, cases, reversed(list(cases)))


def test_interleaved_first_on_a_fresh_handle(world):
    cases = world[3]
    with _engine(world) as eng:            # (no slots yet: the first call allocates 1024, the second regrows them to 8192)
        _run(eng, cases, INTERLEAVED)
        _run(eng, cases, list(cases))


def test_an_exclusion_list_alone_leaves_fewer_rows_than_topn(engine_lib):
    """40 rows, 2 members, 30 excluded: 8 rows are left for top-16, and for top-8 exactly enough."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = np.ascontiguousarray(oracle.mt19937_uniform(40, 40))
    members, gone = [5, 21], [r for r in range(40) if r % 4 != 1][:30]
    assert not set(members) & set(gone)
    s = scores_of(feats, feats[members])
    with CosineEngine(feats) as eng:
        for topn in (16, 8, 7):
            want = expected_scored(s, feats, None, None, members + gone, topn)
            assert len(want[0]) == min(topn, 8)
            _same3(request_call(capi, capi.lib().mi355rec_query_playlist_request, eng._h, rows=members, exclude=gone, topn=topn), want,
                   f"8 rows left for top-{topn}")
