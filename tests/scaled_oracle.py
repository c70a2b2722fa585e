"""What a request with FEATURE SCALES (include/mi355rec_diag.h) must return: the existing oracles applied to scaled arrays.

    scale(feats, a) = (feats * a).astype(float32)          column-wise, one fp32 multiply per value

The cosine request is tests/playlist_labels_oracle.py's on scale(feats, a) with the members scale(members, a); the distance request
is tests/distance_oracle.py's on the same arrays.  The feature filter is evaluated on the UNSCALED rows; exclusion, member rows
and label sets are untouched.  Nothing of the engine is used here."""
import ctypes

import numpy as np

from tests import distance_oracle, playlist_labels_oracle

KEY, MODE, TEMPO, GENRE = 2, 4, 10, 11
ONES = np.ones(12, np.float32)
DROP3 = np.ones(12, np.float32)
DROP3[[KEY, MODE, GENRE]] = 0
GENERAL = np.array([2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0], np.float32)
ONE = np.zeros(12, np.float32)
ONE[TEMPO] = 1
EDGE = np.array([1024, 2.0 ** -20, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1], np.float32)
SCALE_SETS = {"ONES": ONES, "DROP3": DROP3, "GENERAL": GENERAL, "ONE": ONE, "EDGE": EDGE}


def scale(feats, a) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.ascontiguousarray((np.asarray(feats, np.float32) * np.asarray(a, np.float32)).astype(np.float32))


def cosine_scores(feats, members, a, weights=None) -> np.ndarray:
    """The scaled cosine mean of every row (computed once per member set and scale set)."""
    with np.errstate(all="ignore"):
        return playlist_labels_oracle.scores_of(scale(feats, a), scale(np.asarray(members, np.float32).reshape(-1, 12), a), weights)


def cosine_expected(scores, feats, excluded, topn, where=None, labels=None, wanted=None):
    """(ids, scores) from cosine_scores; `feats` are the UNSCALED rows (the filter's)."""
    return playlist_labels_oracle.expected_scored(scores, np.asarray(feats, np.float32), labels, wanted, excluded, topn, where)


def distance_m(feats, members, a) -> np.ndarray:
    return distance_oracle.mean_sqdist(scale(feats, a), scale(np.asarray(members, np.float32).reshape(-1, 12), a))


def distance_expected(m, feats, excluded, topn, where=None, labels=None, wanted=None):
    """(ids, distances) from distance_m; `feats` are the UNSCALED rows (the filter's)."""
    return distance_oracle.expected_from_m(np.asarray(feats, np.float32), m, excluded, topn, where, labels, wanted)


def check(got, want, what=""):
    """Equal ids, bit-equal scores or distances."""
    distance_oracle.check(got, want, what)


def request_call(capi, fn, h, metric, scales, **kw):
    """One raw call of mi355rec_[sharded_]query_{playlist|distance}_request_scaled (`fn`; metric "cosine" or "euclidean") through
    the existing request_call of that metric: returns (rc, ids, values).  `scales`: None (a NULL pointer) or 12 floats, passed
    as they are (the argument-error tests pass NaN and the like)."""
    keep = None if scales is None else np.ascontiguousarray(np.asarray(scales, np.float32).reshape(-1))
    ptr = None if keep is None else keep.ctypes.data_as(ctypes.c_void_p)

    def with_scales(handle, query, result):
        return fn(handle, query, ptr, result)

    if metric == "euclidean":
        return distance_oracle.request_call(capi, with_scales, h, **kw)
    rc, ids, score, _, _ = playlist_labels_oracle.request_call(capi, with_scales, h, **kw)
    return rc, ids, score
