"""What a request with a ROW SET must return (include/mi355rec_diag.h, ROW SETS): the existing oracles with a longer exclusion list.

    MI355REC_ROWSET_EXCLUDE:  excluded = exclude + S
    MI355REC_ROWSET_ONLY:     excluded = exclude + ([0, n) without S)

Every oracle of the family takes an exclusion list of any length (tests/playlist_labels_oracle.py, tests/distance_oracle.py,
tests/prior_oracle.py, tests/scaled_oracle.py; tests/diverse_oracle.py and tests/capped_oracle.py then re-rank the admissible
pool), so nothing new is computed here: this file holds that mapping, the set shapes the tests use and a request_call for the four
_ext entry points.  Nothing of the engine is used for an expectation."""
import ctypes

import numpy as np

from tests import distance_oracle, playlist_labels_oracle, prior_oracle

EXCLUDE, ONLY = 0, 1          # MI355REC_ROWSET_*
MODES = (("exclude", EXCLUDE), ("only", ONLY))


def excluded(n: int, ids, mode: int, exclude=()) -> np.ndarray:
    """The exclusion list that stands for the set `ids` (global rows of a catalogue of n rows, row_base 0) in `mode`, after the
    caller's own `exclude`."""
    inside = np.zeros(n, bool)
    s = np.asarray(list(ids), np.int64).reshape(-1)
    inside[s[(s >= 0) & (s < n)]] = True
    gone = np.flatnonzero(inside if mode == EXCLUDE else ~inside)
    return np.concatenate([np.asarray(list(exclude), np.int64).reshape(-1), gone.astype(np.int64)])


def admitted(n: int, ids, mode: int) -> int:
    """How many rows the set leaves."""
    return n - int(np.unique(excluded(n, ids, mode)).size)


def shapes(n: int, seed: int = 0) -> dict:
    """The fixed set shapes by local row r (name -> int64 ids, unsorted where it matters little; "random30" is seeded)."""
    r = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng([seed, n, 77])
    return {
        "empty": r[:0],
        "all": r,
        "all_but_last": r[:-1],
        "last_only": r[-1:],
        "even": r[r % 2 == 0],
        "low_nibble": r[r % 8 < 4],
        "high_nibble": r[r % 8 >= 4],
        "mod4_is_1": r[r % 4 == 1],
        "random30": r[rng.random(n) < 0.3],
    }


def prefix(expected, topn: int):
    """The top-`topn` of an expectation computed for a larger topn: the canonical order is total, so it is the prefix."""
    return tuple(a[:topn] for a in expected)


def request_call(capi, fn, h, metric, rowset, mode, *, scales=None, ext_size=None, ext_null=False, prior_weight=None, **kw):
    """One raw call of mi355rec_[sharded_]query_{playlist|distance}_request_ext (`fn`; metric "cosine" or "euclidean") through
    the existing request_call of that metric.  `rowset`: None (NULL) or the set's pointer; `mode`: the struct's rowset_mode as it
    is (the argument-error tests pass 2); `scales`: None or 12 floats; `ext_size`: the struct's size field (default sizeof);
    `ext_null`: pass a NULL ext.  Cosine: returns (rc, ids, scores, mmr, pool_rows); euclidean: (rc, ids, distances)."""
    keep = None if scales is None else np.ascontiguousarray(np.asarray(scales, np.float32).reshape(-1))
    ext = capi.RequestExt()
    ext.size = ctypes.sizeof(capi.RequestExt) if ext_size is None else ext_size
    ext.rowset_mode = int(mode)
    ext.feature_scales = None if keep is None else keep.ctypes.data_as(ctypes.c_void_p)
    ext.rowset = rowset

    def with_ext(handle, query, result):
        return fn(handle, query, None if ext_null else ctypes.byref(ext), result)

    if metric == "euclidean":
        return distance_oracle.request_call(capi, with_ext, h, **kw)
    if prior_weight is not None:
        return prior_oracle.request_call(capi, with_ext, h, prior_weight=prior_weight, **kw)
    return playlist_labels_oracle.request_call(capi, with_ext, h, **kw)
