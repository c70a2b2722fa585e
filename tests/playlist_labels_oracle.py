"""What a call of the playlist family with a LABEL SET must return (include/mi355rec_diag.h, PLAYLIST REQUESTS), composed from
the existing checkers: the family's scores over all rows (tests/weighted_oracle.py; every weight 1 is the plain mean bit for
bit), restricted to the admissible rows (label in the set and >= 0, tests/filter_oracle.pass_mask, not excluded, not a member),
in the oracle's canonical order; then tests/diverse_oracle.py / tests/capped_oracle.py on the pool."""
import numpy as np

from tests.capped_oracle import rerank_capped
from tests.diverse_oracle import rerank
from tests.filter_oracle import pass_mask
from tests.playlist_oracle import expected_from_scores
from tests.weighted_oracle import weighted_scores


def scores_of(feats, members, weights=None):
    """The family's score of every row: computed once per member set and shared by the cases that only change the rest."""
    members = np.asarray(members, dtype=np.float32).reshape(-1, 12)
    return weighted_scores(feats, members, np.ones(members.shape[0], np.float32) if weights is None else weights)


def inadmissible(feats, labels, wanted, where=None):
    """The rows the label set and the filter leave out (wanted None: no label set)."""
    bad = ~pass_mask(feats, where)
    if wanted is not None:
        lab = np.asarray(labels)
        bad |= (lab < 0) | ~np.isin(lab, np.asarray(list(wanted), dtype=np.int64))
    return np.flatnonzero(bad)


def expected_scored(scores, feats, labels, wanted, excluded, topn: int, where=None):
    """(ids, scores) of the top-`topn` of the admissible rows, from the scores of every row."""
    ex = np.asarray([] if excluded is None else list(excluded), np.int64)
    return expected_from_scores(scores, np.concatenate([inadmissible(feats, labels, wanted, where), ex]), topn)


def expected(feats, labels, members, wanted, excluded, topn: int, where=None, weights=None):
    return expected_scored(scores_of(feats, members, weights), feats, labels, wanted, excluded, topn, where)


def expected_rows(feats, labels, rows, wanted, exclude, topn: int, where=None, weights=None):
    """The by-row call: the members are rows of `feats`, excluded whatever their label."""
    rows = [int(r) for r in rows]
    return expected(feats, labels, feats[rows], wanted, rows + [int(e) for e in ([] if exclude is None else exclude)], topn, where, weights)


def expected_diverse(pool, feats, lam, topn: int, groups=None, max_per_group=None):
    """(ids, rel, mmr) picked from `pool` = (ids, rel) of the admissible rows' top-`pool`; with groups: capped."""
    pidx, prel = pool
    if pidx.size == 0:
        return np.empty(0, np.int64), np.empty(0, np.float32), np.empty(0, np.float32)
    if groups is None:
        return rerank(feats, pidx, prel, lam, topn)
    return rerank_capped(feats, pidx, prel, groups, lam, max_per_group, topn)


def contiguous_labels(n: int, n_labels: int):
    """Labels in blocks of equal size in row order (a catalogue sorted by genre): whole tiles fail the label test."""
    return (np.arange(n, dtype=np.int64) * n_labels // max(n, 1)).astype(np.int32)


def uniform_labels(n: int, n_labels: int, seed: int, unlabelled: float = 0.02):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, n_labels, size=n).astype(np.int32)
    lab[rng.random(n) < unlabelled] = -1
    return lab


def request_call(capi, fn, h, *, members=None, rows=None, weights=None, exclude=None, where=None, labels=None, n_labels=None, topn=10,
                 lam=None, pool=None, max_per_group=None, size=None, flags=None, k=None, n_exclude=None):
    """One raw call of mi355rec_[sharded_]query_playlist_request (`fn`): returns (rc, ids, scores, mmr, pool_rows), the arrays
    cut at the count.  Fields left None stay zero / NULL; `size`, `flags`, `k`, `n_labels`, `n_exclude` override what the
    other arguments imply (for the argument-error and struct-versioning tests)."""
    import ctypes

    from spotify_recommender_amd.engine import make_filter
    keep = []

    def ptr(a, dtype):
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)

    q = capi.PlaylistQuery()
    q.size = ctypes.sizeof(capi.PlaylistQuery) if size is None else size
    if members is not None:
        m = np.asarray(members, np.float32).reshape(-1, 12)
        q.members, q.k = ptr(m, np.float32), m.shape[0]
    if rows is not None:
        q.rows, q.k = ptr(rows, np.int64), len(rows)
    if weights is not None:
        q.weights = ptr(weights, np.float32)
    if exclude is not None and len(exclude):
        q.exclude_global, q.n_exclude = ptr(exclude, np.int64), len(exclude)
    if where is not None:
        flt = where if isinstance(where, capi.Filter) else make_filter(where)
        keep.append(flt)
        q.filter = ctypes.pointer(flt)
    if labels is not None:
        q.labels, q.n_labels = ptr(list(labels) or [0], np.int32), len(labels)
    q.topn = int(topn)
    q.flags = (capi.PQ_DIVERSE if lam is not None else 0) | (capi.PQ_CAPPED if max_per_group is not None else 0)
    if lam is not None:
        q.lambda_, q.pool = float(lam), int(pool)
    if max_per_group is not None:
        q.max_per_group = int(max_per_group)
    for name, v in (("flags", flags), ("k", k), ("n_labels", n_labels), ("n_exclude", n_exclude)):
        if v is not None:
            setattr(q, name, v)
    n_out = max(int(topn), 1)
    idx, score, mmr = np.full(n_out, -7, np.int64), np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    count, pool_rows = ctypes.c_int(-7), ctypes.c_int(-7)
    res = capi.PlaylistResult(idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p),
                              mmr.ctypes.data_as(ctypes.c_void_p), ctypes.pointer(count), ctypes.pointer(pool_rows))
    rc = fn(h, ctypes.byref(q), ctypes.byref(res))
    c = max(count.value, 0)
    if rc == 0:   # what an accepted call leaves behind the count: -1 / 0 / 0 up to topn, whichever path answered
        assert 0 <= count.value <= n_out and np.all(idx[:c] >= 0), (count.value, idx)
        assert np.all(idx[c:] == -1) and not score[c:].any() and not mmr[c:].any(), (c, idx[c:], score[c:], mmr[c:])
    return rc, idx[:c].copy(), score[:c].copy(), mmr[:c].copy(), pool_rows.value
