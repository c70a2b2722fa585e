"""What a request with a CANDIDATE LIST must return (include/mi355rec_diag.h, CANDIDATE LISTS): the request with an ONLY row set made
from the list, so the existing oracles with a longer exclusion list (tests/rowset_oracle.py):

    list C:                 excluded = exclude + ([0, n) without C)
    list C + EXCLUDE S:     excluded = exclude + ([0, n) without C) + S
    list C + ONLY S:        excluded = exclude + ([0, n) without (C and S))

Nothing new is computed here and nothing of the engine is used for an expectation: this file holds that mapping, the list sizes the
tests use and a request_call for the four _candidates entry points."""
import ctypes

import numpy as np

from tests import rowset_oracle
from tests.rowset_oracle import EXCLUDE, ONLY


def gone(n: int, candidates, exclude=(), rowset=None, mode: int = EXCLUDE) -> np.ndarray:
    """The exclusion list that stands for the list (and a row set `rowset` in `mode`) on a catalogue of n rows, row_base 0."""
    out = rowset_oracle.excluded(n, candidates, ONLY, exclude)
    if rowset is not None:
        out = np.concatenate([out, rowset_oracle.excluded(n, rowset, mode)])
    return out


def distinct_in(candidates, lo: int, hi: int) -> int:
    """The distinct ids of [lo, hi) in the list: what mi355rec_candidates_counters' rows_gathered rises by on that shard."""
    c = np.asarray(list(candidates), np.int64).reshape(-1)
    return int(np.unique(c[(c >= lo) & (c < hi)]).size)


# List entries of one workgroup per iteration of the gather: 512 threads times the entries of a thread, a tuning constant of the
# kernel (csrc/playlist.hip.h, kPlGatherPerThread) that is no part of the interface.  The tests therefore take the edges of every
# value it can sensibly have (1, 2 or 4 entries: an iteration appends at most a tile's 2048 keys), and a retuned kernel stays covered.
CHUNKS = (512, 1024, 2048)


def edge_sizes(n: int) -> list:
    """Distinct in-shard list sizes at which the gather takes another path, up to n: 1, 2, a workgroup's thread edge and its
    iteration edge for every chunk size, and every row."""
    sizes = {1, 2, n}
    for c in CHUNKS:
        sizes |= {c - 1, c, c + 1}
    return sorted(s for s in sizes if 1 <= s <= n)


def request_call(capi, fn, h, metric, candidates, rowset=None, mode=0, *, n_candidates=None, null_list=False, **kw):
    """One raw call of mi355rec_[sharded_]query_{playlist|distance}_request_candidates (`fn`) through rowset_oracle.request_call (so
    `scales`, `ext_size`, `ext_null`, `prior_weight` and the request's own keywords are its).  `candidates`: the ids; `n_candidates`:
    the count passed (default: their number); `null_list`: pass NULL for the list."""
    c = np.ascontiguousarray(np.asarray(list(candidates), np.int64).reshape(-1))
    count = int(c.size) if n_candidates is None else int(n_candidates)
    ptr = None if null_list or c.size == 0 else c.ctypes.data_as(ctypes.c_void_p)

    def as_ext(handle, query, ext, result):
        return fn(handle, query, ext, ptr, count, result)

    return rowset_oracle.request_call(capi, as_ext, h, metric, rowset, mode, **kw)
