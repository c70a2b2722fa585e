"""What a weighted playlist query must return, from the oracle (include/mi355rec_diag.h, WEIGHTED PLAYLISTS): per row the
oracle's score c_k against every member, then in float32, member order, multiply then add (an explicit rounding after
every operation, never fused), one divide:

    W        = fl(...fl(|w_0| + |w_1|) + ... + |w_{K-1}|)
    score(x) = fl( fl(...fl( fl(w_0 c_0) + fl(w_1 c_1) ) + ... + fl(w_{K-1} c_{K-1}) ) / W )

the excluded rows and the rows failing the filter removed, the rest in the oracle's canonical order."""
import numpy as np

from oracle import oracle
from tests.filter_oracle import expected_where
from tests.playlist_oracle import expected_from_scores  # noqa: F401  (re-exported: the ranking of every playlist oracle)


def weight_sum(weights):
    w = np.abs(np.asarray(weights, dtype=np.float32).reshape(-1))
    total = np.float32(w[0])
    for x in w[1:]:
        total = np.float32(total + x)
    return total


def weighted_scores(feats, members, weights):
    members = np.asarray(members, dtype=np.float32).reshape(-1, 12)
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert w.size == members.shape[0]
    total = (w[0] * oracle.scores(feats, np.ascontiguousarray(members[0]))).astype(np.float32)
    for q, wk in zip(members[1:], w[1:]):
        term = (wk * oracle.scores(feats, np.ascontiguousarray(q))).astype(np.float32)
        total = (total + term).astype(np.float32)
    return (total / weight_sum(w)).astype(np.float32)


def expected(feats, members, weights, excluded, topn: int, where=None):
    """(ids, scores) of the weighted top-`topn` for member vectors `members` (k x 12), `excluded` global rows left out."""
    return expected_where(weighted_scores(feats, members, weights), feats, where, excluded, topn)


def expected_rows(feats, rows, weights, exclude, topn: int, where=None):
    """The by-row call: members are rows of `feats`, excluded (whatever their weight) together with `exclude`."""
    rows = [int(r) for r in rows]
    return expected(feats, feats[rows], weights, rows + [int(e) for e in (exclude if exclude is not None else [])], topn, where)


def weight_kinds(rng, k):
    """The three kinds of weights the tests run: positive, signed Gaussian, likes with every third song disliked at -0.5."""
    yield "positive", rng.uniform(0.25, 4.0, k).astype(np.float32)
    yield "signed", rng.normal(0.0, 1.0, k).astype(np.float32)
    yield "dislikes", np.where(np.arange(k) % 3 == 2, -0.5, 1.0).astype(np.float32)
