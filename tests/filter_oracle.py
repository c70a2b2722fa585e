"""What a feature-filtered playlist query must return, from the oracle (tests/playlist_oracle.py): the rows whose features
lie within every active bound (numpy float32 compares, so a NaN feature fails) and are not excluded, ranked by the playlist
score in the oracle's canonical order."""
import ctypes

import numpy as np

from tests.playlist_oracle import expected_from_scores, mean_scores

NAMES = ("danceability", "energy", "key", "loudness", "mode", "speechiness", "acousticness", "instrumentalness", "liveness",
         "valence", "tempo", "genre_id")


def bounds(where):
    """{feature index or name: (lo, hi)} -> (active, lo[12], hi[12]) as float32, ranges on one feature intersected."""
    active, lo, hi = 0, np.full(12, -np.inf, np.float32), np.full(12, np.inf, np.float32)
    for key, (a, b) in dict(where or {}).items():
        j = NAMES.index(key) if isinstance(key, str) else int(key)
        a, b = np.float32(a), np.float32(b)
        if active & (1 << j):
            a, b = max(a, lo[j]), min(b, hi[j])
        active |= 1 << j
        lo[j], hi[j] = a, b
    return active, lo, hi


def pass_mask(feats, where):
    """all(lo <= x <= hi) over the active features, per row (float32)."""
    active, lo, hi = bounds(where)
    ok = np.ones(feats.shape[0], dtype=bool)
    for j in range(12):
        if active & (1 << j):
            ok &= (lo[j] <= feats[:, j]) & (feats[:, j] <= hi[j])
    return ok


def expected_where(scores, feats, where, excluded, topn: int):
    """(ids, scores) of the filtered top-`topn` from the playlist scores of every row."""
    failing = np.flatnonzero(~pass_mask(feats, where))
    return expected_from_scores(scores, np.concatenate([failing, np.asarray(list(excluded), np.int64)]), topn)


def expected(feats, members, excluded, where, topn: int):
    return expected_where(mean_scores(feats, members), feats, where, excluded, topn)


def expected_rows(feats, rows, exclude, where, topn: int):
    rows = [int(r) for r in rows]
    return expected(feats, feats[rows], rows + [int(e) for e in (exclude if exclude is not None else [])], where, topn)


def raw_filter(capi, active, lo=None, hi=None):
    """A capi.Filter with exactly these fields (no checks: for the argument-error tests)."""
    f = capi.Filter()
    f.active = ctypes.c_uint32(active).value
    for j in range(12):
        f.lo[j] = float(lo[j]) if lo is not None else 0.0
        f.hi[j] = float(hi[j]) if hi is not None else 1.0
    return f
