"""What a diversified query must return, from the oracle (include/mi355rec_diag.h, DIVERSIFIED TOP-N).  The pool is the
weighted playlist oracle's top-`pool` (tests/weighted_oracle.py); c(i, p) = oracle.scores(pool rows, feats[p]) (row i scanned,
row p the query); then, in numpy float32 with an explicit rounding after every operation (never fused):

    mu    = fl(1 - lam)                        pen_i = +0.0 at the start
    mmr_i = fl( fl(lam * rel_i) - fl(mu * pen_i) )
    pick the unpicked i with the largest mmr_i (IEEE >; a tie stays with the earlier pool position)
    pen_i = c(i, p) where c(i, p) > pen_i      for every unpicked i

min(topn, P') picks, in pick order; the scores returned are the relevance."""
import numpy as np

from oracle import oracle
from tests.weighted_oracle import expected as pool_expected


def rerank(feats, pool_idx, pool_rel, lam, topn: int):
    """(ids, rel, mmr) of the greedy picks from a pool in canonical order."""
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    rel = np.asarray(pool_rel, dtype=np.float32)
    rows = np.ascontiguousarray(feats[pool_idx])
    p_eff = rel.size
    pen = np.zeros(p_eff, dtype=np.float32)
    picked = np.zeros(p_eff, dtype=bool)
    a = (lam * rel).astype(np.float32)
    out, out_mmr = [], []
    for _ in range(min(int(topn), p_eff)):
        b = (mu * pen).astype(np.float32)
        mmr = (a - b).astype(np.float32)
        # IEEE >, the first wins a tie: argmax returns the first of equal maxima (-0.0 == +0.0); mmr is finite, -inf never wins
        best = int(np.argmax(np.where(picked, -np.inf, mmr.astype(np.float64))))
        picked[best] = True
        out.append(best)
        out_mmr.append(mmr[best])
        c = oracle.scores(rows, np.ascontiguousarray(rows[best]))
        pen = np.where(c > pen, c, pen).astype(np.float32)
    out = np.asarray(out, dtype=np.int64)
    return np.asarray(pool_idx, np.int64)[out], rel[out], np.asarray(out_mmr, dtype=np.float32)


def expected(feats, members, weights, excluded, where, lam, pool: int, topn: int):
    """(ids, rel, mmr) for member vectors `members` (k x 12); weights None: the plain mean (every weight 1)."""
    members = np.asarray(members, dtype=np.float32).reshape(-1, 12)
    w = np.ones(members.shape[0], np.float32) if weights is None else weights
    pidx, prel = pool_expected(feats, members, w, [] if excluded is None else excluded, pool, where)
    return rerank(feats, pidx, prel, lam, topn)


def expected_rows(feats, rows, weights, exclude, where, lam, pool: int, topn: int):
    """The by-row call: members are rows of `feats`, excluded together with `exclude`."""
    rows = [int(r) for r in rows]
    return expected(feats, feats[rows], weights, rows + [int(e) for e in (exclude if exclude is not None else [])], where, lam, pool, topn)


def check3(got, want, what=""):
    """Equal ids, bit-equal relevance, bit-equal mmr."""
    gi, gs, gm = got
    wi, ws, wm = want
    assert gi.tolist() == wi.tolist(), f"{what}: ids differ"
    assert np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)), f"{what}: relevance differs"
    assert np.array_equal(np.asarray(gm, np.float32).view(np.uint32), np.asarray(wm, np.float32).view(np.uint32)), f"{what}: mmr differs"


def default_pool(topn: int) -> int:
    return min(1024, max(topn, 4 * topn))


def mean_pairwise(feats, ids):
    """The mean of c(i, p) over the ordered pairs i != p of a result."""
    rows = np.ascontiguousarray(feats[np.asarray(ids, np.int64)])
    total, n = 0.0, len(ids)
    for p in range(n):
        c = oracle.scores(rows, np.ascontiguousarray(rows[p])).astype(np.float64)
        total += c.sum() - c[p]
    return total / (n * (n - 1))


# ---- the parity grid the CPU and GPU suites share ------------------------------------------------------------------------
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
LAMBDAS = (0.0, 0.3, 0.5, 0.7, 1.0)


def pools(topn):
    return sorted({topn, min(4 * topn, 1024), 1024})


def variants(rng, feats, k):
    """(name, by-row rows or None, member vectors, weights, exclusion list, filter): with and without each extra."""
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    vecs = rng.random((k, 12), dtype=np.float32)
    excl = rng.integers(0, feats.shape[0], size=300)
    dislikes = np.where(np.arange(k) % 3 == 2, -0.5, 1.0).astype(np.float32)   # (k < 3: likes only)
    signed = rng.normal(0.0, 1.0, k).astype(np.float32)
    signed[0] = -abs(signed[0]) - np.float32(0.1)                               # a dislike for every k
    yield "by row", rows, None, None, None, None
    yield "by value", None, vecs, None, None, None
    yield "by row, dislikes", rows, None, dislikes, None, None
    yield "by value, signed weights, excluded, filtered", None, vecs, signed, excl, WHERE
    yield "by row, excluded, filtered", rows, None, None, excl, WHERE


def run_variant(nd, feats, v, lam, pool, topn):
    """The variant through any engine object (CosineEngine, a lane, NodeEngine): (ids, rel, mmr)."""
    name, rows, vecs, w, excl, where = v
    if rows is not None:
        return nd.query_playlist_topn_diverse(rows, topn, lam, pool, exclude=excl, where=where, weights=w, return_mmr=True)
    return nd.query_mean_topn_diverse(vecs, topn, lam, pool, exclude=excl, where=where, weights=w, return_mmr=True)


def variant_pool(feats, v, pool):
    """The oracle's pool of a variant (it does not depend on lambda)."""
    name, rows, vecs, w, excl, where = v
    members = feats[rows] if rows is not None else vecs
    excluded = ([int(r) for r in rows] if rows is not None else []) + ([] if excl is None else [int(e) for e in excl])
    return pool_expected(feats, members, np.ones(len(members), np.float32) if w is None else w, excluded, pool, where)
