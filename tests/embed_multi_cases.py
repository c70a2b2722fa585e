"""Interests, requests and the numpy statement of MULTI-INTEREST EMBEDDING REQUESTS (include/mi355rec_embed_multi.h) for the
CPU and the GPU tests: per interest the v of tests/embed_cases.expected (the family's oracle, tests/embed_oracle.py), then
V = the largest finite v_k per row and the lowest k that gives it, then embed_oracle.topn over V; and the merge of identity 2
over K single-interest answers."""
import numpy as np

from tests import embed_cases as ec
from tests import embed_oracle as eo

F32 = np.float32
MAX_INTERESTS = 32


def interest_counts(P):
    """K in {1, 2, P - 1, P, P + 1, 2P + 1, 32} for a chunk width P: every way a last chunk can be short."""
    return sorted({k for k in (1, 2, P - 1, P, P + 1, 2 * P + 1, MAX_INTERESTS) if 1 <= k <= MAX_INTERESTS})


def interests(K, d, seed=0):
    """K random interests; from K = 3 on the second is the first again (equal values at two interests)."""
    rng = np.random.default_rng(900 * d + K + seed)
    us = rng.standard_normal((K, d), dtype=F32)
    if K >= 3:
        us[1] = us[0]
    return us


def per_interest(feats, wide, us, req, row_base=0, ranked=True):
    """v_k of every row [K, n]: embed_cases.expected's v with u = interest k (req: metric, weights, the audio side).
    ranked=False takes the same v from embed_oracle.values, where embed_cases.expected takes it, without the top-N that
    expected computes beside it (a table of millions of rows need not be sorted K times for a v that is then maximised)."""
    base = {k: val for k, val in req.items() if k not in ("topn", "exclude", "user", "rows")}
    if ranked:
        return np.stack([ec.expected(feats, wide, dict(base, user=u, topn=1), row_base)[0] for u in us]).astype(F32)
    audio = base.get("audio")
    if audio is None and "audio_row" in base:
        audio = feats[base["audio_row"]]
    metric = eo.DOT if base["metric"] == "dot" else eo.COSINE
    return np.stack([eo.values(wide, u, metric, base["embed_weight"], base.get("audio_weight", 0.0), feats, audio)[0] for u in us]).astype(F32)


def best(vs):
    """(V [n], interest [n]) of v_k [K, n]: V is NaN and the interest -1 where no v_k is finite."""
    vs = np.asarray(vs, F32)
    fin = np.isfinite(vs)
    masked = np.where(fin, vs, F32(-np.inf))
    k = (masked == masked.max(axis=0)[None, :]).argmax(axis=0).astype(np.int32)   # (the first: -0.0 == +0.0)
    V = vs[k, np.arange(vs.shape[1])]                                             # (that interest's own bits)
    has = fin.any(axis=0)
    return np.where(has, V, F32(np.nan)).astype(F32), np.where(has, k, np.int32(-1)).astype(np.int32)


def expected(feats, wide, us, req, row_base=0, topn=eo.topn, ranked=True):
    """(ids, scores, interests, vs) of a request: the oracle's answer."""
    vs = per_interest(feats, wide, us, req, row_base, ranked)
    V, k = best(vs)
    ids, sc = topn(V, req["topn"], req.get("exclude", ()), row_base)
    return ids, sc, k[ids - row_base], vs


def merge(answers, n_top):
    """Identity 2: answers[k] = (ids, scores) of interest k's single request, merged: union by row, the larger value kept, the
    lower k preferred at equal values, ordered by value descending then id ascending, the first n_top."""
    held = {}
    for k, (ids, sc) in enumerate(answers):
        for i, s in zip(np.asarray(ids).tolist(), np.asarray(sc, F32)):
            if i not in held or s > held[i][0]:
                held[i] = (s, k)
    rows = np.array(sorted(held), np.int64)
    vals = np.array([held[i][0] for i in rows.tolist()], F32) + F32(0)
    ks = np.array([held[i][1] for i in rows.tolist()], np.int32)
    order = np.lexsort((rows, -vals.astype(np.float64)))[:n_top]
    return rows[order], vals[order], ks[order]


def hostile_exclusions(n, L, row_base=0, seed=0):
    """L global ids: rows of the table in any order with duplicates, foreign and negative ids among them."""
    if L == 0:
        return []
    rng = np.random.default_rng(31 * n + L + seed)
    ids = [int(x) + row_base for x in rng.integers(-3, n + 4, L)]
    extra = [row_base, row_base, row_base + n - 1, row_base + n, -1, 2 ** 31 + 7, 2 ** 40]
    for j, x in enumerate(extra[: max(L // 2, 1)]):
        ids[(7 * j) % L] = x
    return ids
