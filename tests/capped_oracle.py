"""What a capped query must return, from the oracle (include/mi355rec_diag.h, GROUP CAPS): the diversified oracle
(tests/diverse_oracle.py: the same pool, c(i, p), mu, pen and mmr in numpy float32 with one rounding per operation) with
the eligibility rule: an unpicked pool row may be picked iff its group is -1 or fewer than `max_per_group` picked rows share
its group; the loop ends after `topn` picks or when nothing is eligible.  Also the closed form for lambda = 1 (the pool rows
whose rank inside their group within the pool is below the cap, the first `topn` of them)."""
import numpy as np

from oracle import oracle
from tests.diverse_oracle import WHERE, check3, pools, variant_pool, variants  # noqa: F401  (re-exported: the shared grid)


def rerank_capped(feats, pool_idx, pool_rel, groups, lam, max_per_group: int, topn: int):
    """(ids, rel, mmr) of the greedy picks from a pool in canonical order; groups: one id per catalogue row."""
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    rel = np.asarray(pool_rel, dtype=np.float32)
    pool_idx = np.asarray(pool_idx, np.int64)
    rows = np.ascontiguousarray(feats[pool_idx])
    g = np.asarray(groups, dtype=np.int64)[pool_idx]
    p_eff = rel.size
    pen = np.zeros(p_eff, dtype=np.float32)
    picked = np.zeros(p_eff, dtype=bool)
    seen = np.zeros(p_eff, dtype=np.int64)       # per pool row: the picked rows of its group
    a = (lam * rel).astype(np.float32)
    out, out_mmr = [], []
    for _ in range(min(int(topn), p_eff)):
        eligible = ~picked & ((g < 0) | (seen < int(max_per_group)))
        if not eligible.any():
            break
        b = (mu * pen).astype(np.float32)
        mmr = (a - b).astype(np.float32)
        # IEEE >, the first wins a tie: argmax returns the first of equal maxima; mmr is finite, -inf never wins
        best = int(np.argmax(np.where(eligible, mmr.astype(np.float64), -np.inf)))
        picked[best] = True
        if g[best] >= 0:
            seen += g == g[best]
        out.append(best)
        out_mmr.append(mmr[best])
        c = oracle.scores(rows, np.ascontiguousarray(rows[best]))
        pen = np.where(c > pen, c, pen).astype(np.float32)
    out = np.asarray(out, dtype=np.int64)
    return pool_idx[out], rel[out], np.asarray(out_mmr, dtype=np.float32)


def in_order_capped(pool_idx, pool_rel, groups, max_per_group: int, topn: int):
    """The closed form for lambda = 1: (ids, rel, mmr = rel)."""
    pool_idx = np.asarray(pool_idx, np.int64)
    rel = np.asarray(pool_rel, dtype=np.float32)
    g = np.asarray(groups, dtype=np.int64)[pool_idx]
    count, keep = {}, []
    for i, gi in enumerate(g.tolist()):
        rank = count.get(gi, 0)
        count[gi] = rank + 1
        if gi < 0 or rank < int(max_per_group):
            keep.append(i)
    keep = np.asarray(keep[:int(topn)], dtype=np.int64)
    return pool_idx[keep], rel[keep], rel[keep].copy()


def cap_holds(ids, groups, max_per_group: int) -> bool:
    g = np.asarray(groups, dtype=np.int64)[np.asarray(ids, np.int64)]
    g = g[g >= 0]
    return g.size == 0 or int(np.unique(g, return_counts=True)[1].max()) <= int(max_per_group)


def default_pool(topn: int) -> int:
    return min(1024, max(topn, 8 * topn))


def layouts(n: int, seed: int = 5):
    """{name: one int32 group per row}: the layouts the CPU and GPU suites share."""
    rows = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    mixed = (rows * 2654435761 % 97).astype(np.int32)
    mixed[rng.random(n) < 1.0 / 3.0] = -1
    return {
        "row % 7": (rows % 7).astype(np.int32),                       # the cap binds hard: count < topn occurs
        "row // 3": (rows // 3).astype(np.int32),
        "all -1": np.full(n, -1, np.int32),
        "a third -1": mixed,
        "near 2^31": (np.int64(2 ** 31 - 1) - rows % 5).astype(np.int32),
    }


def run_variant(nd, v, lam, pool, max_per_group, topn):
    """The variant through any engine object: (ids, rel, mmr, pool_rows)."""
    name, rows, vecs, w, excl, where = v
    if rows is not None:
        return nd.query_playlist_topn_capped(rows, topn, max_per_group, lam, pool, exclude=excl, where=where, weights=w, return_mmr=True,
                                             return_pool_rows=True)
    return nd.query_mean_topn_capped(vecs, topn, max_per_group, lam, pool, exclude=excl, where=where, weights=w, return_mmr=True,
                                     return_pool_rows=True)


def check4(got, want3, pool_rows, what=""):
    """Equal ids, bit-equal relevance, bit-equal mmr (hence the count) and P'."""
    check3(got[:3], want3, what)
    assert got[3] == pool_rows, f"{what}: pool_rows {got[3]}, expected {pool_rows}"
