"""What a playlist query must return, from the oracle: per row the oracle's score against every member, summed in float32
in member order and divided once by float32(K), the excluded rows removed, the rest in the oracle's canonical order
(score descending, then row ascending)."""
import numpy as np

from oracle import oracle


def mean_scores(feats, members):
    """score(x) = fl(fl(...fl(c_0 + c_1) + ... + c_{K-1}) / K) for every row x (float32)."""
    members = np.asarray(members, dtype=np.float32).reshape(-1, 12)
    total = oracle.scores(feats, np.ascontiguousarray(members[0]))
    for q in members[1:]:
        total = (total + oracle.scores(feats, np.ascontiguousarray(q))).astype(np.float32)
    return (total / np.float32(len(members))).astype(np.float32)


def expected_from_scores(scores, excluded, topn: int):
    keep = np.ones(scores.size, dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    keep[ex[(ex >= 0) & (ex < scores.size)]] = False
    sel = np.flatnonzero(keep)
    if sel.size == 0:
        return np.empty(0, np.int64), np.empty(0, np.float32)
    idx, sc = oracle.topn_canonical(np.ascontiguousarray(scores[sel]), -1, topn)
    return sel[idx].astype(np.int64), sc + np.float32(0)


def expected(feats, members, excluded, topn: int):
    """(ids, scores) of the playlist top-`topn` for member vectors `members` (k x 12), `excluded` global rows left out."""
    return expected_from_scores(mean_scores(feats, members), excluded, topn)


def expected_rows(feats, rows, exclude, topn: int):
    """The by-row call: members are rows of `feats`, excluded together with `exclude`."""
    rows = [int(r) for r in rows]
    return expected(feats, feats[rows], rows + [int(e) for e in (exclude or [])], topn)
