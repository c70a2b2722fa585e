"""Users, exclusion lists and the one check of the USER BATCH tests (include/mi355rec_embed_batch.h): every user's ids,
score bits, padding and count against tests/embed_oracle.py — the contract of mi355rec_embed_query with w_audio = 0 —
per user and bit for bit.  Tables come from tests/embed_cases.catalogue (duplicates, hostile rows)."""
import itertools

import numpy as np

from tests import embed_oracle as eo

F32 = np.float32
BATCHES = [1, 2, 7, 8, 9, 17]   # a full pass of 8, short last passes, the pass boundary
METRICS = ["cosine", "dot"]
WEIGHTS = [1.0, -0.5, 4.0]


def topns(n):
    return [1, 10, 128, min(n + 5, 128)]


def combos(n):
    """Every (metric, embed_weight, topn) of the sweep, 24 of them."""
    return list(itertools.product(METRICS, WEIGHTS, topns(n)))


def users(n, d, count, seed=0):
    rng = np.random.default_rng(31 * d + n + 1000 * count + seed)
    return rng.standard_normal((count, d), dtype=F32)


def sweep_lists(n, count):
    """Exclusion lists of a sweep batch: every third user none (an EMPTY list between full ones), the others duplicates,
    foreign ids (>= n, >= 2^31, negative) and rows of the table."""
    out = []
    for b in range(count):
        out.append([] if b % 3 == 1 else [0, 0, n - 1, n + 5, 2 ** 31 + 7, -4, n // 2, (b * 7) % n])
    return out


def expected(table, u, metric, w_embed, topn, exclude=(), row_base=0):
    """(ids [topn] -1 padded, scores [topn] 0 padded, count) of one user by the oracle."""
    v, _ = eo.values(table, u, eo.DOT if metric == "dot" else eo.COSINE, w_embed)
    ids, sc = eo.topn(v, topn, exclude, row_base)
    pad_i = np.full(topn, -1, np.int64)
    pad_s = np.zeros(topn, F32)
    pad_i[: ids.size] = ids
    pad_s[: ids.size] = sc
    return pad_i, pad_s, ids.size


def check(tab, table, us, *, topn, metric, embed_weight, exclude=None, row_base=0, what=""):
    """One call for all of `us`, every user against the oracle; returns what the call returned."""
    before = tab.info()
    ids, sc, counts = tab.query_users(users=us, topn=topn, metric=metric, embed_weight=embed_weight, exclude=exclude)
    after = tab.info()
    B = len(us)
    assert ids.shape == (B, topn) and sc.shape == (B, topn) and counts.shape == (B,)
    assert after["users_served"] - before["users_served"] == B, what
    assert after["passes"] - before["passes"] == -(-B // after["pass_users"]), f"{what}: {B} users took {after['passes'] - before['passes']} passes"
    for b in range(B):
        wi, ws, wc = expected(table, us[b], metric, embed_weight, topn, exclude[b] if exclude is not None else (), row_base)
        tag = f"{what} user {b} of {B} ({metric}, w {embed_weight}, top-{topn})"
        assert counts[b] == wc, f"{tag}: count {counts[b]}, want {wc}"
        assert ids[b].tolist() == wi.tolist(), f"{tag}: ids differ (got {ids[b][:8].tolist()}, want {wi[:8].tolist()})"
        assert np.array_equal(eo.bits(sc[b]), eo.bits(ws)), f"{tag}: score bits differ"
    return ids, sc, counts
