"""What a JACCARD REQUEST (include/mi355rec_diag.h) must return, computed here in numpy and by nothing of the engine.

The contract's chain, one rounded fp32 operation per step, rows vectorised, members in order:
    num = den = 0.0f
    for j = 0..11:  lt = x_j < q_kj;  lo = lt ? x_j : q_kj;  hi = lt ? q_kj : x_j;  num = fl(num + lo);  den = fl(den + hi)
    J_k  = fl(num / den)
    v(x) = fl( fl(...fl(J_0 + J_1) + ... + J_{K-1}) / (float)K )
min and max are np.where on the ONE compare x < q (np.minimum / np.maximum propagate a NaN from either side; the contract sends a
NaN of the row to den and a NaN of a member to num).  Rows are ranked by v descending, then row ascending; a row whose v is not
finite or one of whose den_k is not below +inf, an excluded row, a row failing the feature filter, outside the label set or not
admitted by the row set is not admissible; the reported value is v (-0.0 as +0.0, as the keys carry it).

`cross_check` compares the chain with float64 on NON-NEGATIVE inputs: every term of num and den is then non-negative, so each
sum's error is relative to itself: at most 11 ulp each (the first add is exact), the divide 1 more: J_k within 23 ulp of its real
value; the K - 1 adds over the members (each J_k in [0, 1], so the partial sums are non-negative) and the divide add K more.
|v32 - v64| <= (K + 26) ulp of v64 + 2^-140, ulp = 2^-24 relative, with 3 ulp of room."""
import ctypes

import numpy as np

from tests.distance_oracle import hostile_catalogue as _distance_hostile
from tests.distance_oracle import pass_mask

ULP = np.float64(2.0 ** -24)


def hostile_catalogue(n: int, seed: int = 5):
    """The distance oracle's hostile rows (NaN, +inf, -inf, an all-zero row, a row of 1e-30, a row of 1e30, duplicates of row 0 at
    8, 9, 10, n // 2 and n - 1) and, from row 11 on where they fit: a row with negative features of mixed sign, a row that is the
    negative of row 0 (exactly -1 against row 0) and an all-negative row (against an all-zero member: den = 0)."""
    f = _distance_hostile(n, seed)
    if n > 14:
        f[11, ::2] = -f[11, ::2]
        f[12] = -f[0]
        f[13] = -np.abs(f[13]) - np.float32(0.25)
    return np.ascontiguousarray(f)


def mean_jaccard(feats, members):
    """(v, valid) of every row: v float32, bit for bit the contract's chain; valid: the row may form a key (v finite and every
    den_k below +inf)."""
    f = np.ascontiguousarray(feats, np.float32)
    q = np.ascontiguousarray(members, np.float32).reshape(-1, 12)
    total = None
    valid = np.ones(f.shape[0], bool)
    with np.errstate(all="ignore"):
        for k in range(q.shape[0]):
            num = np.zeros(f.shape[0], np.float32)
            den = np.zeros(f.shape[0], np.float32)
            for j in range(12):
                x = f[:, j]
                lt = x < q[k, j]
                num = (num + np.where(lt, x, q[k, j]).astype(np.float32)).astype(np.float32)
                den = (den + np.where(lt, q[k, j], x).astype(np.float32)).astype(np.float32)
            valid &= den < np.float32(np.inf)
            jk = (num / den).astype(np.float32)
            total = jk if total is None else (total + jk).astype(np.float32)
        v = (total / np.float32(q.shape[0])).astype(np.float32)
    return v, valid & np.isfinite(v)


def cross_check(feats, members, v32, valid) -> None:
    f = np.asarray(feats, np.float64)
    q = np.asarray(members, np.float64).reshape(-1, 12)
    k = q.shape[0]
    with np.errstate(all="ignore"):
        v64 = np.mean([np.minimum(q[i], f).sum(axis=1) / np.maximum(q[i], f).sum(axis=1) for i in range(k)], axis=0)
        # (non-negative rows and members whose sums stay normal fp32 numbers: what the bound above is about)
        ok = valid & np.isfinite(v64) & np.all(f >= 0, axis=1) & np.all(f < 1e30, axis=1) & bool(np.all(q >= 0) and np.all(q < 1e30))
        ok &= np.all((f == 0) | (f > 1e-25), axis=1)
        err = np.abs(v32.astype(np.float64)[ok] - v64[ok])
        bound = (k + 26) * ULP * v64[ok] + 2.0 ** -140
    assert np.all(err <= bound), f"the fp32 chain is {np.max(err / bound):.3g} x the float64 bound away"
    assert np.all((v32[ok] >= 0) & (v32[ok] <= 1)), "the Ruzicka similarity of non-negative vectors lies in [0, 1]"


def admissible(feats, valid, excluded=(), where=None, labels=None, wanted=None, rowset=None, rowset_only=False) -> np.ndarray:
    ok = np.array(valid, bool)
    ex = np.asarray([int(e) for e in excluded if 0 <= int(e) < len(ok)], np.int64)
    ok[ex] = False
    if where is not None:
        ok &= pass_mask(np.asarray(feats, np.float32), where)
    if wanted is not None:
        ok &= np.isin(labels, np.asarray(list(wanted), np.int64)) & (np.asarray(labels) >= 0)
    if rowset is not None:
        inside = np.zeros(len(ok), bool)
        inside[np.asarray([int(r) for r in rowset if 0 <= int(r) < len(ok)], np.int64)] = True
        ok &= inside if rowset_only else ~inside
    return ok


def expected_from_v(feats, v_valid, excluded, topn, where=None, labels=None, wanted=None, rowset=None, rowset_only=False):
    """(ids, similarities) of the `topn` most similar admissible rows from (v, valid) of every row; v = -0.0 is reported as +0.0."""
    v, valid = v_valid
    ok = admissible(feats, valid, excluded, where, labels, wanted, rowset, rowset_only)
    rows = np.flatnonzero(ok)
    key = (v[rows] + np.float32(0)).astype(np.float32)
    order = np.lexsort((rows, -key.astype(np.float64)))[:topn]   # (float64 negation: exact, and -0.0 has gone)
    ids = rows[order].astype(np.int64)
    return ids, (v[ids] + np.float32(0)).astype(np.float32)


def expected(feats, members, excluded, topn, **kw):
    return expected_from_v(feats, mean_jaccard(feats, members), excluded, topn, **kw)


def expected_rows(feats, rows, excluded, topn, **kw):
    rows = [int(r) for r in rows]
    return expected(feats, np.asarray(feats, np.float32)[rows], rows + [int(e) for e in (excluded or [])], topn, **kw)


def check(got, want, what=""):
    """Equal ids, bit-equal similarities."""
    gi, gs = got
    wi, ws = want
    assert np.asarray(gi).tolist() == np.asarray(wi).tolist(), f"{what}: ids differ: {np.asarray(gi)[:8]} vs {np.asarray(wi)[:8]}"
    assert np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)), f"{what}: similarities differ"


def request_call(capi, fn, h, *, members=None, rows=None, exclude=None, where=None, labels=None, n_labels=None, topn=10, size=None,
                 flags=None, k=None, n_exclude=None, ext=None, want_similarity=True):
    """One raw call of mi355rec_[sharded_]query_jaccard_request (`fn`) with the output buffers filled with 7s first: returns
    (rc, ids, similarities), the arrays cut at the count; on success asserts count in [0, topn] and -1 / +0.0f past it.  Fields
    left None stay zero / NULL; `size`, `flags`, `k`, `n_labels`, `n_exclude` override what the other arguments imply.
    `ext`: a capi.RequestExt or None."""
    from spotify_recommender_amd.engine import make_filter

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    keep = []
    q = capi.JaccardQuery()
    q.size = ctypes.sizeof(capi.JaccardQuery) if size is None else size
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
    idx, sim = np.full(n_out, 7, np.int64), np.full(n_out, 7, np.float32)
    c = ctypes.c_int(-5)
    res = capi.JaccardResult(ptr(idx), ptr(sim) if want_similarity else None, ctypes.pointer(c))
    rc = fn(h, ctypes.byref(q), ctypes.byref(ext) if ext is not None else None, ctypes.byref(res))
    if rc != capi.OK:
        return rc, idx[:0], sim[:0]
    n = c.value
    assert 0 <= n <= topn, f"count {n} for topn {topn}"
    assert np.all(idx[:n] >= 0) and np.all(idx[n:topn] == -1), f"ids around the count {n}: {idx[:topn]}"
    if want_similarity:
        assert not sim[n:topn].view(np.uint32).any(), f"similarities past the count {n}"
    return rc, idx[:n].copy(), sim[:n].copy()
