"""What a CANDIDATE SCORES call must return (include/mi355rec_diag.h, CANDIDATE SCORES): for every listed id, in list order, the
value the existing CPU oracles give that row (tests/playlist_labels_oracle.py, tests/scaled_oracle.py, tests/prior_oracle.py,
tests/distance_oracle.py), or the quiet NaN 0x7fc00000 with flag 0 where the row can never be returned.  Nothing new is computed here
and nothing of the engine is used for an expectation: this file holds that mapping and a score_call for the four scoring entry points."""
import ctypes

import numpy as np

from tests import rowset_oracle

QUIET_NAN = 0x7FC00000


def expected(n: int, handed, values, gone=(), distance: bool = False):
    """(value bits uint32[len(handed)], flags bool[...]).  `values`: the oracle's score (or m, with distance=True) of every row of a
    catalogue of n rows, row_base 0; `gone`: every row that is not admissible for another reason (excluded ids, members given by row,
    what playlist_labels_oracle.inadmissible and rowset_oracle.excluded name).  A distance is admissible only where m is finite and
    reports as sqrt(m) in float32; a score of -0.0 reports as +0.0."""
    ids = np.asarray(list(handed), np.int64).reshape(-1)
    ok_row = np.ones(n, bool)
    g = np.asarray(list(gone), np.int64).reshape(-1)
    ok_row[g[(g >= 0) & (g < n)]] = False
    v = np.asarray(values, np.float32)
    with np.errstate(all="ignore"):
        if distance:
            ok_row &= np.isfinite(v)
            v = np.sqrt(v).astype(np.float32)
        v = (v + np.float32(0)).astype(np.float32)
    inside = (ids >= 0) & (ids < n)
    flags = np.zeros(ids.size, bool)
    flags[inside] = ok_row[ids[inside]]
    bits = np.full(ids.size, QUIET_NAN, np.uint32)
    bits[flags] = v[ids[flags]].view(np.uint32)
    return bits, flags


def check(got, want, what=""):
    """Equal flags, bit-equal values (the NaN of an inadmissible entry included)."""
    gv, gf = got
    wb, wf = want
    assert np.asarray(gf).astype(bool).tolist() == np.asarray(wf).astype(bool).tolist(), f"{what}: flags differ"
    gb = np.asarray(gv, np.float32).view(np.uint32)
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:4]}: {gb[bad[:4]]} vs {wb[bad[:4]]}"


def score_call(capi, fn, h, metric, candidates, rowset=None, mode=0, *, n_candidates=None, null_list=False, null_value=False,
               null_flags=False, **kw):
    """One raw call of mi355rec_[sharded_]score_{playlist|distance}_request_candidates (`fn`; metric "cosine" or "euclidean") with the
    query and ext that rowset_oracle.request_call builds (its keywords).  Returns (rc, values float32, flags uint8); both arrays are
    filled with 7s first, so what the call leaves alone shows."""
    c = np.ascontiguousarray(np.asarray(list(candidates), np.int64).reshape(-1))
    count = int(c.size) if n_candidates is None else int(n_candidates)
    values = np.full(max(c.size, 1), 7.0, np.float32)
    flags = np.full(max(c.size, 1), 7, np.uint8)
    rc = []

    def as_ext(handle, query, ext, result):
        rc.append(fn(handle, query, ext, None if null_list or c.size == 0 else c.ctypes.data_as(ctypes.c_void_p), count,
                     None if null_value else values.ctypes.data_as(ctypes.c_void_p),
                     None if null_flags else flags.ctypes.data_as(ctypes.c_void_p)))
        return capi.ERR_INVALID_ARG   # (the wrapped request_call then checks nothing of the result buffers it made)

    rowset_oracle.request_call(capi, as_ext, h, metric, rowset, mode, **kw)
    return rc[0], values[:c.size], flags[:c.size]
