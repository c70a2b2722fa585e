"""What a label-filtered query must return, from the oracle: the oracle's scores restricted to the rows whose label is in
the set, in the oracle's canonical order (score descending, then row ascending), the query row excluded by index."""
import numpy as np

from oracle import oracle


def expected(feats, labels, query, exclude: int, wanted, topn: int):
    """(ids, scores) of the filtered top-`topn` for the query vector `query`."""
    return expected_from_scores(oracle.scores(feats, query), labels, exclude, wanted, topn)


def expected_from_scores(scores, labels, exclude: int, wanted, topn: int):
    sel = np.flatnonzero(np.isin(labels, np.asarray(list(wanted), dtype=np.int32)))
    sub_exclude = -1
    if exclude >= 0:
        hit = np.searchsorted(sel, exclude)
        if hit < sel.size and sel[hit] == exclude:
            sub_exclude = int(hit)
    if sel.size == 0:
        return np.empty(0, np.int64), np.empty(0, np.float32)
    idx, sc = oracle.topn_canonical(np.ascontiguousarray(scores[sel]), sub_exclude, topn)
    return sel[idx].astype(np.int64), sc + np.float32(0)


def check(got, want, what=""):
    gi, gs = got
    wi, ws = want
    assert gi.tolist() == wi.tolist(), f"{what}: ids differ"
    assert np.array_equal(np.asarray(gs, np.float32).view(np.uint32), np.asarray(ws, np.float32).view(np.uint32)), f"{what}: scores differ"


def catalogue(rows: int, n_labels: int, seed: int, unlabelled: float = 0.02):
    """A uniform random catalogue with random labels in [0, n_labels) (a few rows -1), plus the rows that make ties and
    degenerate scores: zero rows and exact duplicates, labelled 3 and 5 (inside the sets the tests ask for)."""
    feats = oracle.mt19937_uniform(seed, rows)
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_labels, size=rows).astype(np.int32)
    labels[rng.random(rows) < unlabelled] = -1
    feats[10:14] = 0.0                  # zero rows: score 0 against everything
    labels[10:14] = 3
    feats[100:110] = feats[99]          # duplicates of row 99: equal scores, ties broken by row
    labels[99:110] = 5
    labels[200:205] = 5
    feats[200:205] = feats[99] * 2.0    # (scaled copies: the same cosine up to rounding)
    return np.ascontiguousarray(feats), labels
