"""What a DISTANCE REQUEST (include/mi355rec_diag.h) must return, computed here in numpy and by nothing of the engine.

The contract's chain, one rounded fp32 operation per step, rows vectorised, members in order:
    d2_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fl(t * t))      (acc starts at 0.0f)
    m(x)    = fl( fl(...fl(d2_0 + d2_1) + ... + d2_{K-1}) / (float)K )
Rows are ranked by m ascending, then row ascending (lexsort on (row, m)); a row whose m is not finite, an excluded row, a row
failing the feature filter or outside the label set is not admissible; the reported value is sqrt(m) in fp32.

`cross_check` compares the chain with float64: for rows whose float64 value is finite and below the fp32 range,
|m32 - m64| <= 64 ulp of (m64 + Q2) + 2^-120, ulp = 2^-24 relative and Q2 = mean |q_k|^2.  (Every term of the chain is
non-negative, so its error is relative to m itself: about 16 ulp.  The absolute 2^-120 is the room for squares that underflow
in fp32 — rows and members of 1e-30 — where nothing relative holds.)"""
import ctypes

import numpy as np

from tests.filter_oracle import pass_mask

ULP = np.float64(2.0 ** -24)


def mean_sqdist(feats, members) -> np.ndarray:
    """m(x) of every row: float32, bit for bit the contract's chain."""
    f = np.ascontiguousarray(feats, np.float32)
    q = np.ascontiguousarray(members, np.float32).reshape(-1, 12)
    total = None
    with np.errstate(all="ignore"):
        for k in range(q.shape[0]):
            acc = np.zeros(f.shape[0], np.float32)
            for j in range(12):
                t = (q[k, j] - f[:, j]).astype(np.float32)
                acc = (acc + (t * t).astype(np.float32)).astype(np.float32)
            total = acc if total is None else (total + acc).astype(np.float32)
        return (total / np.float32(q.shape[0])).astype(np.float32)


def cross_check(feats, members, m32) -> None:
    f = np.asarray(feats, np.float64)
    q = np.asarray(members, np.float64).reshape(-1, 12)
    with np.errstate(all="ignore"):
        m64 = np.mean([((q[k] - f) ** 2).sum(axis=1) for k in range(q.shape[0])], axis=0)
        q2 = np.mean((q ** 2).sum(axis=1))
        ok = np.isfinite(m64) & (m64 < 1e37) & np.isfinite(q2)
        err = np.abs(m32.astype(np.float64)[ok] - m64[ok])
        bound = 64 * ULP * (m64[ok] + q2) + 2.0 ** -120
    assert np.all(err <= bound), f"the fp32 chain is {np.max(err / bound):.3g} x the float64 bound away"


def admissible(feats, m, excluded=(), where=None, labels=None, wanted=None) -> np.ndarray:
    ok = np.isfinite(m)
    ex = np.asarray([int(e) for e in excluded if 0 <= int(e) < len(m)], np.int64)
    ok[ex] = False
    if where is not None:
        ok &= pass_mask(np.asarray(feats, np.float32), where)
    if wanted is not None:
        ok &= np.isin(labels, np.asarray(list(wanted), np.int64)) & (np.asarray(labels) >= 0)
    return ok


def expected_from_m(feats, m, excluded, topn, where=None, labels=None, wanted=None):
    """(ids, distances) of the `topn` nearest admissible rows from m(x) of every row."""
    ok = admissible(feats, m, excluded, where, labels, wanted)
    rows = np.flatnonzero(ok)
    order = np.lexsort((rows, m[rows]))[:topn]
    ids = rows[order].astype(np.int64)
    with np.errstate(all="ignore"):
        return ids, np.sqrt(m[ids]).astype(np.float32)


def expected(feats, members, excluded, topn, where=None, labels=None, wanted=None):
    return expected_from_m(feats, mean_sqdist(feats, members), excluded, topn, where, labels, wanted)


def expected_rows(feats, rows, excluded, topn, where=None, labels=None, wanted=None):
    rows = [int(r) for r in rows]
    return expected(feats, np.asarray(feats, np.float32)[rows], rows + [int(e) for e in (excluded or [])], topn, where, labels, wanted)


def check(got, want, what=""):
    """Equal ids, bit-equal distances."""
    gi, gd = got
    wi, wd = want
    assert np.asarray(gi).tolist() == np.asarray(wi).tolist(), f"{what}: ids differ: {np.asarray(gi)[:8]} vs {np.asarray(wi)[:8]}"
    assert np.array_equal(np.asarray(gd, np.float32).view(np.uint32), np.asarray(wd, np.float32).view(np.uint32)), f"{what}: distances differ"


def hostile_catalogue(n: int, seed: int = 5):
    """Uniform rows with, from row 2 on where they fit: NaN, +inf, -inf, an all-zero row, a row of 1e-30, a row of 1e30 (its
    square overflows), and duplicates of row 0 (ties by row)."""
    f = np.random.default_rng([seed, n]).random((n, 12), dtype=np.float32)
    specials = [("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)]
    at = 2
    for _, v in specials:
        if at < n:
            f[at, at % 12] = v
        at += 1
    for v in (0.0, 1e-30, 1e30):
        if at < n:
            f[at] = np.float32(v)
        at += 1
    for d in range(at, min(at + 3, n)):
        f[d] = f[0]
    if n > 40:
        f[n - 1] = f[0]
        f[n // 2] = f[0]
    return np.ascontiguousarray(f)


def request_call(capi, fn, h, *, members=None, rows=None, exclude=None, where=None, labels=None, n_labels=None, topn=10, size=None,
                 flags=None, k=None, n_exclude=None):
    """One raw call of mi355rec_[sharded_]query_distance_request (`fn`) with the output buffers filled with 7s first: returns
    (rc, ids, distances), the arrays cut at the count; on success asserts count in [0, topn] and -1 / +0.0f past it.  Fields left
    None stay zero / NULL; `size`, `flags`, `k`, `n_labels`, `n_exclude` override what the other arguments imply."""
    from spotify_recommender_amd.engine import make_filter

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    keep = []
    q = capi.DistanceQuery()
    q.size = ctypes.sizeof(capi.DistanceQuery) if size is None else size
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
    res = capi.DistanceResult(ptr(idx), ptr(dist), ctypes.pointer(c))
    rc = fn(h, ctypes.byref(q), ctypes.byref(res))
    if rc != capi.OK:
        return rc, idx[:0], dist[:0]
    n = c.value
    assert 0 <= n <= topn, f"count {n} for topn {topn}"
    assert np.all(idx[:n] >= 0) and np.all(idx[n:topn] == -1), f"ids around the count {n}: {idx[:topn]}"
    assert not dist[n:topn].view(np.uint32).any(), f"distances past the count {n}"
    return rc, idx[:n].copy(), dist[:n].copy()
