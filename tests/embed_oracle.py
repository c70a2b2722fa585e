"""The numpy statement of the EMBEDDING TABLE contract (include/mi355rec_embed.h): tree sums in float32, c, v, and the
expected ids, scores and padding of a request.  Every product and every sum is a float32 numpy operation of its own, so
nothing is fused; sqrt and divide are numpy's correctly rounded float32 ones.  The audio cosine s(x) is the project's
oracle (oracle/oracle.py)."""
import numpy as np

from oracle import oracle

COSINE, DOT = 0, 1
F32 = np.float32


def tree(a, b):
    """tree(a, b) per row: a [n, d], b [d] or [n, d] -> [n] float32."""
    with np.errstate(all="ignore"):
        a = np.asarray(a, F32)
        pr = a * np.asarray(b, F32)                 # each product rounded on its own
        p = pr[:, 0::4] + pr[:, 1::4]
        p = p + pr[:, 2::4]
        p = p + pr[:, 3::4]                         # p_g
        while p.shape[1] > 1:
            p = p[:, 0::2] + p[:, 1::2]             # t(l+1)_g = fl(t_2g + t_2g+1)
        return p[:, 0]


def user_from_rows(table, rows):
    """u = e_r0, then u = fl(u + e_rk) in list order."""
    with np.errstate(all="ignore"):
        u = np.array(table[rows[0]], F32)
        for r in rows[1:]:
            u = u + table[r]
        return u


def similarity(table, u, metric):
    """c of every row."""
    with np.errstate(all="ignore"):
        table = np.asarray(table, F32)
        u = np.asarray(u, F32)
        dot = tree(table, u)
        if metric == DOT:
            return dot
        nu = np.sqrt(tree(u[None, :], u))[0]
        den = np.sqrt(tree(table, table)) * nu
        t = dot / den
        m = np.where(t < F32(1), t, F32(1))
        c = np.where(F32(-1) < m, m, F32(-1))
        return np.where(den > F32(1e-8), c, F32(0)).astype(F32)


def values(table, u, metric, w_embed, w_audio=0.0, feats=None, audio=None):
    """(v, c) of every row; audio: the 12 floats of the audio query (needed when w_audio != 0)."""
    with np.errstate(all="ignore"):
        c = similarity(table, u, metric)
        b = F32(w_embed) * c
        if F32(w_audio) == 0:
            return b.astype(F32), c
        s = oracle.scores(np.ascontiguousarray(feats, F32), np.ascontiguousarray(audio, F32))
        a = F32(w_audio) * s
        return (a + b).astype(F32), c


def topn(v, n_top, exclude=(), row_base=0):
    """The expected (ids, scores) of a request: finite v only, excluded global ids left out, v descending then row ascending,
    -0.0 reported as +0.0."""
    v = np.asarray(v, F32)
    ok = np.isfinite(v)
    for x in exclude:
        if row_base <= x < row_base + v.size:
            ok[int(x) - row_base] = False
    rows = np.nonzero(ok)[0]
    vv = v[rows] + F32(0)
    order = np.lexsort((rows, -vv.astype(np.float64)))[:n_top]
    return rows[order].astype(np.int64) + row_base, vv[order]


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)
