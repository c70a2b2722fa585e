"""What a MANHATTAN REQUEST (include/mi355rec_diag.h) must return, computed here in numpy and by nothing of the engine.

The contract's chain, one rounded fp32 operation per step, rows vectorised, members in order:
    d1_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fabsf(t))      (acc starts at 0.0f)
    m(x)    = fl( fl(...fl(d1_0 + d1_1) + ... + d1_{K-1}) / (float)K )
Rows are ranked by m ascending, then row ascending (lexsort on (row, m)); a row whose m is not finite, an excluded row, a row
failing the feature filter, outside the label set or not admitted by the row set is not admissible; the reported value is m.

`cross_check` compares the chain with float64: for rows whose float64 value is finite and below the fp32 range,
|m32 - m64| <= (K + 16) ulp of m64 + 2^-140, ulp = 2^-24 relative.  Every term of the chain is non-negative, so its error is
relative to m itself: the subtraction 1 ulp of its term, the twelve adds at most 12 of d1_k, the K - 1 adds over the members
and the divide K more: K + 13, with 3 ulp of room.  A difference that is subnormal is exact in IEEE arithmetic, so nothing
absolute is lost; 2^-140 only keeps the comparison meaningful at m64 = 0."""
import ctypes

import numpy as np

from tests.distance_oracle import admissible as _admissible
from tests.distance_oracle import hostile_catalogue  # noqa: F401  (the tests take it from here)

ULP = np.float64(2.0 ** -24)


def mean_l1(feats, members) -> np.ndarray:
    """m(x) of every row: float32, bit for bit the contract's chain."""
    f = np.ascontiguousarray(feats, np.float32)
    q = np.ascontiguousarray(members, np.float32).reshape(-1, 12)
    total = None
    with np.errstate(all="ignore"):
        for k in range(q.shape[0]):
            acc = np.zeros(f.shape[0], np.float32)
            for j in range(12):
                t = (q[k, j] - f[:, j]).astype(np.float32)
                acc = (acc + np.abs(t)).astype(np.float32)
            total = acc if total is None else (total + acc).astype(np.float32)
        return (total / np.float32(q.shape[0])).astype(np.float32)


def cross_check(feats, members, m32) -> None:
    f = np.asarray(feats, np.float64)
    q = np.asarray(members, np.float64).reshape(-1, 12)
    k = q.shape[0]
    with np.errstate(all="ignore"):
        m64 = np.mean([np.abs(q[i] - f).sum(axis=1) for i in range(k)], axis=0)
        ok = np.isfinite(m64) & (m64 < 1e37)
        err = np.abs(m32.astype(np.float64)[ok] - m64[ok])
        bound = (k + 16) * ULP * m64[ok] + 2.0 ** -140
    assert np.all(err <= bound), f"the fp32 chain is {np.max(err / bound):.3g} x the float64 bound away"


def admissible(feats, m, excluded=(), where=None, labels=None, wanted=None, rowset=None, rowset_only=False) -> np.ndarray:
    ok = _admissible(feats, m, excluded, where, labels, wanted)
    if rowset is not None:
        inside = np.zeros(len(m), bool)
        inside[np.asarray([int(r) for r in rowset if 0 <= int(r) < len(m)], np.int64)] = True
        ok &= inside if rowset_only else ~inside
    return ok


def expected_from_m(feats, m, excluded, topn, where=None, labels=None, wanted=None, rowset=None, rowset_only=False):
    """(ids, distances) of the `topn` nearest admissible rows from m(x) of every row; m = 0 is reported as +0.0."""
    ok = admissible(feats, m, excluded, where, labels, wanted, rowset, rowset_only)
    rows = np.flatnonzero(ok)
    order = np.lexsort((rows, m[rows]))[:topn]
    ids = rows[order].astype(np.int64)
    return ids, (m[ids] + np.float32(0)).astype(np.float32)


def expected(feats, members, excluded, topn, **kw):
    return expected_from_m(feats, mean_l1(feats, members), excluded, topn, **kw)


def expected_rows(feats, rows, excluded, topn, **kw):
    rows = [int(r) for r in rows]
    return expected(feats, np.asarray(feats, np.float32)[rows], rows + [int(e) for e in (excluded or [])], topn, **kw)


def check(got, want, what=""):
    """Equal ids, bit-equal distances."""
    gi, gd = got
    wi, wd = want
    assert np.asarray(gi).tolist() == np.asarray(wi).tolist(), f"{what}: ids differ: {np.asarray(gi)[:8]} vs {np.asarray(wi)[:8]}"
    assert np.array_equal(np.asarray(gd, np.float32).view(np.uint32), np.asarray(wd, np.float32).view(np.uint32)), f"{what}: distances differ"


def request_call(capi, fn, h, *, members=None, rows=None, exclude=None, where=None, labels=None, n_labels=None, topn=10, size=None,
                 flags=None, k=None, n_exclude=None, ext=None, want_distance=True):
    """One raw call of mi355rec_[sharded_]query_manhattan_request (`fn`) with the output buffers filled with 7s first: returns
    (rc, ids, distances), the arrays cut at the count; on success asserts count in [0, topn] and -1 / +0.0f past it.  Fields left
    None stay zero / NULL; `size`, `flags`, `k`, `n_labels`, `n_exclude` override what the other arguments imply.
    `ext`: a capi.RequestExt or None."""
    from spotify_recommender_amd.engine import make_filter

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    keep = []
    q = capi.ManhattanQuery()
    q.size = ctypes.sizeof(capi.ManhattanQuery) if size is None else size
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
    idx, dist = np.full(n_out, 7, np.int64), np.full(n_out, 7, np.float32)
    c = ctypes.c_int(-5)
    res = capi.ManhattanResult(ptr(idx), ptr(dist) if want_distance else None, ctypes.pointer(c))
    rc = fn(h, ctypes.byref(q), ctypes.byref(ext) if ext is not None else None, ctypes.byref(res))
    if rc != capi.OK:
        return rc, idx[:0], dist[:0]
    n = c.value
    assert 0 <= n <= topn, f"count {n} for topn {topn}"
    assert np.all(idx[:n] >= 0) and np.all(idx[n:topn] == -1), f"ids around the count {n}: {idx[:topn]}"
    if want_distance:
        assert not dist[n:topn].view(np.uint32).any(), f"distances past the count {n}"
    return rc, idx[:n].copy(), dist[:n].copy()
