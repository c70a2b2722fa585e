"""What an ANY-OF REQUEST (include/mi355rec_diag.h) must return, computed here in numpy and by nothing of the engine.

The contract, rows vectorised, members in order:
    c_k(x) = the oracle's single-query score of row x for q_k          (oracle.scores: core.hip.h's chain, one rounded fp32
                                                                        operation per step; never NaN, in [-1, 1])
    v(x) = c_0;  a(x) = 0;   for k = 1 .. K-1:  if (c_k > v) { v = c_k; a = k; }        (IEEE compare: -0.0 does not beat +0.0)
Rows rank by v descending, then row ascending; the reported score is v with -0.0 as +0.0; a is the smallest member index that
attains the maximum.  A row is admissible iff it is not excluded, passes the feature filter, has its label in the label set and is
admitted by the row set."""
import ctypes

import numpy as np

from oracle import oracle
from tests.filter_oracle import pass_mask


def member_scores(feats, members) -> np.ndarray:
    """c[k, x]: float32 [K, n]."""
    f = np.ascontiguousarray(feats, np.float32)
    q = np.ascontiguousarray(members, np.float32).reshape(-1, 12)
    return np.stack([oracle.scores(f, np.ascontiguousarray(q[k])) for k in range(q.shape[0])]).astype(np.float32)


def best_of(c):
    """(v, a) of every row from c[k, x]: the contract's compare chain."""
    v = c[0].copy()
    a = np.zeros(c.shape[1], np.int32)
    for k in range(1, c.shape[0]):
        better = c[k] > v
        v = np.where(better, c[k], v).astype(np.float32)
        a = np.where(better, np.int32(k), a).astype(np.int32)
    return v, a


def value(feats, members):
    return best_of(member_scores(feats, members))


def admissible(feats, n, excluded=(), where=None, labels=None, wanted=None, rowset=None, rowset_only=False) -> np.ndarray:
    ok = np.ones(n, bool)
    ex = np.asarray([int(e) for e in excluded if 0 <= int(e) < n], np.int64)
    ok[ex] = False
    if where is not None:
        ok &= pass_mask(np.asarray(feats, np.float32), where)
    if wanted is not None:
        ok &= np.isin(labels, np.asarray(list(wanted), np.int64)) & (np.asarray(labels) >= 0)
    if rowset is not None:
        inside = np.zeros(n, bool)
        inside[np.asarray([int(r) for r in rowset if 0 <= int(r) < n], np.int64)] = True
        ok &= inside if rowset_only else ~inside
    return ok


def expected_from_v(feats, v, a, excluded, topn, where=None, labels=None, wanted=None, rowset=None, rowset_only=False):
    """(ids, scores, member) of the `topn` best admissible rows from v(x) and a(x) of every row."""
    ok = admissible(feats, v.size, excluded, where, labels, wanted, rowset, rowset_only)
    rows = np.flatnonzero(ok)
    order = np.lexsort((rows, -v[rows]))[:topn]      # (-0.0 and +0.0 compare equal: ties by row, as the packed keys do)
    ids = rows[order].astype(np.int64)
    return ids, (v[ids] + np.float32(0)).astype(np.float32), a[ids].astype(np.int32)


def expected(feats, members, excluded, topn, **kw):
    v, a = value(feats, members)
    return expected_from_v(feats, v, a, excluded, topn, **kw)


def expected_rows(feats, rows, excluded, topn, **kw):
    rows = [int(r) for r in rows]
    return expected(feats, np.asarray(feats, np.float32)[rows], rows + [int(e) for e in (excluded or [])], topn, **kw)


def check(got, want, what=""):
    """Equal ids, bit-equal scores, equal member indices."""
    gi, gs, gm = got
    wi, ws, wm = want
    assert np.asarray(gi).tolist() == np.asarray(wi).tolist(), f"{what}: ids differ: {np.asarray(gi)[:8]} vs {np.asarray(wi)[:8]}"
    assert np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)), f"{what}: scores differ"
    assert np.asarray(gm).tolist() == np.asarray(wm).tolist(), f"{what}: members differ: {np.asarray(gm)[:8]} vs {np.asarray(wm)[:8]}"


def request_call(capi, fn, h, *, members=None, rows=None, exclude=None, where=None, labels=None, n_labels=None, topn=10, size=None,
                 flags=None, k=None, n_exclude=None, ext=None, want_member=True, want_score=True):
    """One raw call of mi355rec_[sharded_]query_anyof_request (`fn`) with the output buffers filled with 7s first: returns
    (rc, ids, scores, member), the arrays cut at the count; on success asserts count in [0, topn] and -1 / +0.0f / -1 past it.
    Fields left None stay zero / NULL; `size`, `flags`, `k`, `n_labels`, `n_exclude` override what the other arguments imply.
    `ext`: a capi.RequestExt or None."""
    from spotify_recommender_amd.engine import make_filter

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    keep = []
    q = capi.AnyOfQuery()
    q.size = ctypes.sizeof(capi.AnyOfQuery) if size is None else size
    q.flags = 0 if flags is None else flags
    if members is not None:
        m = np.ascontiguousarray(np.asarray(members, np.float32).reshape(-1, 12))
        keep.append(m)
        q.members, q.k = ptr(m), m.shape[0]
    if rows is not None:
        r = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1))
        keep.append(r)
        q.rows, q.k = ptr(r), r.size
    if exclude is not None:
        e = np.ascontiguousarray(np.asarray(list(exclude), np.int64).reshape(-1))
        keep.append(e)
        q.exclude_global, q.n_exclude = (ptr(e) if e.size else None), e.size
    if where is not None:
        flt = make_filter(where)
        keep.append(flt)
        q.filter = ctypes.pointer(flt)
    if labels is not None:
        lab = np.ascontiguousarray(np.asarray(list(labels), np.int32).reshape(-1))
        keep.append(lab)
        q.labels, q.n_labels = ptr(lab), lab.size
    if n_labels is not None:
        q.n_labels = n_labels
    if k is not None:
        q.k = k
    if n_exclude is not None:
        q.n_exclude = n_exclude
    q.topn = topn
    n_out = max(int(topn), 1)
    idx, sc, mem = np.full(n_out, 7, np.int64), np.full(n_out, 7, np.float32), np.full(n_out, 7, np.int32)
    c = ctypes.c_int(-5)
    res = capi.AnyOfResult(ptr(idx), ptr(sc) if want_score else None, ptr(mem) if want_member else None, ctypes.pointer(c))
    rc = fn(h, ctypes.byref(q), ctypes.byref(ext) if ext is not None else None, ctypes.byref(res))
    if rc != capi.OK:
        return rc, idx[:0], sc[:0], mem[:0]
    n = c.value
    assert 0 <= n <= topn, f"count {n} for topn {topn}"
    assert np.all(idx[:n] >= 0) and np.all(idx[n:topn] == -1), f"ids around the count {n}: {idx[:topn]}"
    if want_score:
        assert not sc[n:topn].view(np.uint32).any(), f"scores past the count {n}"
    if want_member:
        assert np.all(mem[:n] >= 0) and np.all(mem[n:topn] == -1), f"members around the count {n}: {mem[:topn]}"
    return rc, idx[:n].copy(), sc[:n].copy(), mem[:n].copy()
