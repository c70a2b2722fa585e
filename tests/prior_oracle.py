"""What a playlist request with a ROW PRIOR must return (include/mi355rec_diag.h, ROW PRIORS), composed from the existing
checkers: the family's score s of every row (tests/playlist_labels_oracle.scores_of, i.e. tests/weighted_oracle.py), blended as

    v = float32(s + float32(beta * p))          (float32, multiply, round, add, round)

restricted to the admissible rows and put in the oracle's canonical order (v descending, then row ascending) by
tests/playlist_labels_oracle.expected_scored; then tests/diverse_oracle.py / tests/capped_oracle.py on the pool, rel = v."""
import ctypes

import numpy as np

from tests.playlist_labels_oracle import expected_diverse, expected_scored, scores_of  # noqa: F401  (re-exported)

MAX_PRIOR_WEIGHT = 4.0


def blended(scores, priors, beta):
    """v of every row from the family's scores."""
    s = np.asarray(scores, np.float32)
    b = (np.float32(beta) * np.asarray(priors, np.float32)).astype(np.float32)
    return (s + b).astype(np.float32)


def expected_prior(scores, priors, beta, feats, labels, wanted, excluded, topn: int, where=None):
    """(ids, v) of the top-`topn` admissible rows by v; beta None: no prior."""
    v = scores if beta is None else blended(scores, priors, beta)
    return expected_scored(v, feats, labels, wanted, excluded, topn, where)


def prior_kinds(rng, n: int):
    """The prior mixes of the issue's measurements: uniform, skewed (rand^4) and signed."""
    return {"uniform": rng.random(n, dtype=np.float32),
            "skewed": (rng.random(n, dtype=np.float32) ** 4).astype(np.float32),
            "signed": (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)}


def request_call(capi, fn, h, *, members=None, rows=None, weights=None, exclude=None, where=None, labels=None, topn=10, lam=None,
                 pool=None, max_per_group=None, prior_weight=None, size=None, flags=None):
    """One raw call of mi355rec_[sharded_]query_playlist_request (`fn`) with the prior's flag and field: returns
    (rc, ids, scores, mmr, pool_rows), the arrays cut at the count.  prior_weight None: neither the flag nor the field is set;
    `size` and `flags` override what the other arguments imply."""
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
        flt = make_filter(where)
        keep.append(flt)
        q.filter = ctypes.pointer(flt)
    if labels is not None:
        q.labels, q.n_labels = ptr(list(labels), np.int32), len(labels)
    q.topn = int(topn)
    q.flags = (capi.PQ_DIVERSE if lam is not None else 0) | (capi.PQ_CAPPED if max_per_group is not None else 0)
    if lam is not None:
        q.lambda_, q.pool = float(lam), int(pool)
    if max_per_group is not None:
        q.max_per_group = int(max_per_group)
    if prior_weight is not None:
        q.flags |= capi.PQ_PRIOR
        q.prior_weight = prior_weight
    if flags is not None:
        q.flags = flags
    n_out = max(int(topn), 1)
    idx, score, mmr = np.full(n_out, -7, np.int64), np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    count, pool_rows = ctypes.c_int(-7), ctypes.c_int(-7)
    res = capi.PlaylistResult(idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p),
                              mmr.ctypes.data_as(ctypes.c_void_p), ctypes.pointer(count), ctypes.pointer(pool_rows))
    rc = fn(h, ctypes.byref(q), ctypes.byref(res))
    c = max(count.value, 0)
    if rc == 0:   # what an accepted call leaves behind the count: -1 / 0 / 0 up to topn
        assert 0 <= count.value <= n_out and np.all(idx[:c] >= 0), (count.value, idx)
        assert np.all(idx[c:] == -1) and not score[c:].any() and not mmr[c:].any(), (c, idx[c:], score[c:], mmr[c:])
        assert not np.any(np.signbit(score[:c]) & (score[:c] == 0)), "-0.0 reported"
    return rc, idx[:c].copy(), score[:c].copy(), mmr[:c].copy(), pool_rows.value
