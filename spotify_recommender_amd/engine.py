"""Host-side plumbing over the C-ABI: device memory via torch, streams, RCCL.

`CosineEngine` owns one catalogue shard on one GPU.  `ShardedEngine` is the
multi-GPU path required by BASELINE.json's north_star: one process per GPU,
rows sharded contiguously, ONE all-gather of `topn` packed keys per rank per
query over RCCL, then the same device merge kernel that merges the
per-workgroup lists.  No arithmetic happens in Python.
"""
from __future__ import annotations

import ctypes
import types
import weakref
from typing import Optional, Tuple

import numpy as np

from . import capi


def _np_f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _np_labels(labels) -> np.ndarray:
    """A label array or set (int32, contiguous): one label per row for set_labels, the wanted labels for a query."""
    return np.ascontiguousarray(np.asarray(list(labels) if isinstance(labels, (set, frozenset)) else labels, dtype=np.int32).reshape(-1))


def _labels_query(fn, h, check, head, labels, topn: int) -> Tuple[np.ndarray, np.ndarray]:
    """Runs one filtered query entry point: fn(h, *head, labels, n_labels, topn, idx, score, &count)."""
    lab = _np_labels(labels)
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    score = np.empty(n_out, dtype=np.float32)
    count = ctypes.c_int(0)
    check(fn(h, *head, lab.ctypes.data_as(ctypes.c_void_p), int(lab.size), int(topn), idx.ctypes.data_as(ctypes.c_void_p),
             score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)))
    return idx[:count.value].copy(), score[:count.value].copy()


def make_filter(where) -> capi.Filter:
    """mi355rec_filter_t from a `where=` mapping {feature index (0..11) or name (capi.FEATURE_NAMES): (lo, hi)}: a row passes
    iff lo <= x[j] <= hi for every named feature (the stored fp32 values, e.g. [0, 1] for the drop-in's normalised
    catalogue).  A feature named twice (by index and by name) keeps the intersection of its ranges; an empty intersection
    is passed on as lo > hi, which the library refuses."""
    f = capi.Filter()
    for j in range(capi.DIM):
        f.lo[j], f.hi[j] = -np.inf, np.inf
    for key, rng in dict(where).items():
        if isinstance(key, str):
            if key.lower() not in capi.FEATURE_NAMES:
                raise ValueError(f"unknown feature {key!r}: one of {', '.join(capi.FEATURE_NAMES)}")
            j = capi.FEATURE_NAMES.index(key.lower())
        else:
            j = int(key)
            if not 0 <= j < capi.DIM:
                raise ValueError(f"feature index {j} out of [0, {capi.DIM})")
        lo, hi = (float(np.float32(v)) for v in rng)
        if f.active & (1 << j):
            lo, hi = max(lo, f.lo[j]), min(hi, f.hi[j])
        f.active |= 1 << j
        f.lo[j], f.hi[j] = lo, hi
    return f


def make_scales(scales) -> np.ndarray:
    """The 12 float32 FEATURE SCALES (include/mi355rec_diag.h) from a `scales=` argument: a sequence of 12 floats, or a mapping
    {feature index (0..11) or name (capi.FEATURE_NAMES): scale} with every feature it does not name at 1.0.  The library checks
    the values (finite, in [0, capi.MAX_FEATURE_SCALE], not all zero)."""
    if isinstance(scales, dict) or hasattr(scales, "items"):
        a = np.ones(capi.DIM, dtype=np.float32)
        for key, v in dict(scales).items():
            if isinstance(key, str):
                if key.lower() not in capi.FEATURE_NAMES:
                    raise ValueError(f"unknown feature {key!r}: one of {', '.join(capi.FEATURE_NAMES)}")
                j = capi.FEATURE_NAMES.index(key.lower())
            else:
                j = int(key)
                if not 0 <= j < capi.DIM:
                    raise ValueError(f"feature index {j} out of [0, {capi.DIM})")
            a[j] = np.float32(v)
        return a
    a = np.ascontiguousarray(np.asarray(scales, dtype=np.float32).reshape(-1))
    if a.size != capi.DIM:
        raise ValueError(f"{a.size} scales: one per feature, {capi.DIM} in all")
    return a


def _ptr(a):
    """A numpy array's data as the void pointer the C-ABI takes."""
    return a.ctypes.data_as(ctypes.c_void_p)


def _fill_query(q, members, topn: int, exclude, where, labels) -> tuple:
    """Fills what the request structs share (capi.PlaylistQuery, DistanceQuery, AnyOfQuery, ManhattanQuery, JaccardQuery): size, the members by
    value (a (k, 12) float32 array) or by row (a 1-D int64 array), the exclusion list, the filter (make_filter), the label set, k and
    topn.  Returns what the struct now points to: the caller holds it until the call has returned."""
    flt = make_filter(where) if where is not None else None
    ex = np.ascontiguousarray(np.asarray([] if exclude is None else list(exclude), dtype=np.int64).reshape(-1))
    lab = _np_labels(labels) if labels is not None else None
    q.size = ctypes.sizeof(type(q))
    q.members, q.rows = (None, _ptr(members)) if members.dtype == np.int64 else (_ptr(members), None)
    q.exclude_global, q.n_exclude = (_ptr(ex) if ex.size else None), int(ex.size)
    q.filter = ctypes.pointer(flt) if flt is not None else None
    if lab is not None:
        q.labels, q.n_labels = _ptr(lab), int(lab.size)   # (an empty set stays a non-NULL pointer: the library refuses it)
    q.k, q.topn = int(members.shape[0]), int(topn)
    return members, flt, ex, lab


def _call_request(lib, prefix: str, h, check, kind: str, q, res, scales=None, rowset=None, candidates=None) -> None:
    """One top-N request of `kind` through the entry point its arguments need.  "playlist" and "distance": with `candidates` (a
    sequence of global ids) `prefix`query_`kind`_request_candidates, else with `rowset` = (pointer, mode) ..._request_ext, else with
    `scales` (checked: make_scales) ..._request_scaled, else ..._request.  "anyof", "manhattan", "bounded" and "jaccard" have the one entry point
    `prefix`query_`kind`_request, which takes the ext (NULL without a row set) and no scales or list."""
    entry = f"{prefix}query_{kind}_request"
    if kind in ("anyof", "manhattan", "bounded", "jaccard"):
        ext = _request_ext(None, rowset)
        check(getattr(lib, entry)(h, ctypes.byref(q), ctypes.byref(ext) if rowset is not None else None, ctypes.byref(res)))
    elif candidates is not None:
        cand = _np_ids(candidates)
        ext = _request_ext(scales, rowset)
        check(getattr(lib, entry + "_candidates")(h, ctypes.byref(q), ctypes.byref(ext), _ptr(cand) if cand.size else None, int(cand.size),
                                                  ctypes.byref(res)))
    elif rowset is not None:
        ext = _request_ext(scales, rowset)
        check(getattr(lib, entry + "_ext")(h, ctypes.byref(q), ctypes.byref(ext), ctypes.byref(res)))
    elif scales is not None:
        check(getattr(lib, entry + "_scaled")(h, ctypes.byref(q), _ptr(scales), ctypes.byref(res)))
    else:
        check(getattr(lib, entry)(h, ctypes.byref(q), ctypes.byref(res)))


_PLAYLIST_LEVELS = ("", "_where", "_weighted", "_diverse", "_capped")   # each level's entry point takes the previous one's arguments and its own


def _playlist_family(lib, prefix: str, h, check, members, topn: int, exclude=None, where=None, weights=None, level: str = None,
                     lam=None, pool=None, max_per_group=None, return_mmr: bool = False, return_pool_rows: bool = False, labels=None,
                     prior_weight=None, scales=None, rowset=None, candidates=None):
    """Runs one entry point of the playlist family: `prefix`query_{mean|playlist}_topn`level`.  `members` is a (k, 12) float32
    array (by value: mean) or a 1-D int64 array of rows (by row: playlist).  `level` None: the lowest that takes the
    arguments given ("" plain, "_where" with a filter, "_weighted" with weights); "_diverse" and "_capped" are asked for.
    The C argument list, in order: h, members, [weights or NULL: from _weighted on], k, exclude, n_exclude, [filter or NULL:
    from _where on], [lambda, pool: from _diverse on], [max_per_group: _capped], topn, idx, score, [mmr: from _diverse on],
    &count, [&pool_rows: _capped].

    `where`: FEATURE FILTERS (make_filter).  `weights`: one float per member, any sign (WEIGHTED PLAYLISTS).
    DIVERSIFIED TOP-N: `lam` in [0, 1] (1: relevance only); `pool`: how many of the most relevant rows the picks are made
    from, None = min(1024, max(topn, 4 * topn)) (8 * topn capped).  Results come in pick order; the scores are the relevance;
    with return_mmr a third array holds the mmr value of each pick.
    GROUP CAPS: `lam` = 1.0 is relevance order with at most `max_per_group` results per group.  With return_pool_rows the last
    element is pool_rows: fewer than `topn` ids with pool_rows == pool means the pool ran out (raise `pool`), with
    pool_rows < pool that the catalogue has no more.
    PLAYLIST REQUESTS: `labels`, a set of labels (set_labels), restricts the answer (and a diversified call's pool) to rows whose
    label is in it; the call then goes through `prefix`query_playlist_request, the family's one struct-taking entry point.
    None takes exactly the entry point described above.
    ROW PRIORS: `prior_weight` = beta ranks by score + beta * prior (set_priors; |beta| <= capi.MAX_PRIOR_WEIGHT, negative demotes);
    the call goes through the request as well, the returned scores are the blended values.  None takes the entry point used today.
    FEATURE SCALES: `scales` (make_scales) weighs or ignores features; the call goes through `prefix`query_playlist_request_scaled,
    which refuses diversified and capped calls and priors.  None takes the entry point used today.
    ROW SETS: `rowset` = (the set's pointer, capi.ROWSET_EXCLUDE or capi.ROWSET_ONLY); the call goes through
    `prefix`query_playlist_request_ext.  None takes the entry point used today.
    CANDIDATE LISTS: `candidates`, a sequence of global ids (any order, duplicates fine; empty: nothing is returned): only the
    listed rows are gathered and ranked, through `prefix`query_playlist_request_candidates, with whatever else is asked (a
    `rowset` too: both must admit a row).  None takes the entry point used today."""
    if prior_weight is not None and (isinstance(prior_weight, bool) or not isinstance(prior_weight, (int, float, np.integer, np.floating))):
        raise ValueError(f"prior_weight must be a number or None, got {prior_weight!r}")
    if level is None:
        level = "_weighted" if weights is not None else "_where" if where is not None else ""
    rank = _PLAYLIST_LEVELS.index(level)
    diverse, capped = rank >= 3, rank == 4
    if capped and (isinstance(max_per_group, bool) or not isinstance(max_per_group, (int, np.integer))):
        raise ValueError(f"max_per_group must be an integer, got {max_per_group!r}")
    if diverse:
        if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)):
            raise ValueError(f"lam must be a number in [0, 1], got {lam!r}")
        if pool is None:
            pool = min(1024, max(int(topn), (8 if capped else 4) * int(topn)))
        elif isinstance(pool, bool) or not isinstance(pool, (int, np.integer)):
            raise ValueError(f"pool must be an integer or None, got {pool!r}")
    k = int(members.shape[0])
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if w.size != k:
            raise ValueError(f"{w.size} weights for {k} songs: one weight per song")
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    score = np.empty(n_out, dtype=np.float32)
    mmr = np.zeros(n_out, dtype=np.float32)
    count, pool_rows = ctypes.c_int(0), ctypes.c_int(0)
    if labels is not None or prior_weight is not None or scales is not None or rowset is not None or candidates is not None:
        q = capi.PlaylistQuery()
        keep = _fill_query(q, members, topn, exclude, where, labels)   # noqa: F841  (alive until the call has returned)
        q.flags = (capi.PQ_DIVERSE if diverse else 0) | (capi.PQ_CAPPED if capped else 0)
        if prior_weight is not None:
            q.flags |= capi.PQ_PRIOR
            q.prior_weight = float(prior_weight)
        q.weights = _ptr(w) if w is not None else None
        if diverse:
            q.lambda_, q.pool = float(lam), int(pool)
        if capped:
            q.max_per_group = int(max_per_group)
        res = capi.PlaylistResult(_ptr(idx), _ptr(score), _ptr(mmr) if diverse else None, ctypes.pointer(count), ctypes.pointer(pool_rows))
        _call_request(lib, prefix, h, check, "playlist", q, res, make_scales(scales) if scales is not None else None, rowset, candidates)
    else:
        flt = make_filter(where) if where is not None else None
        ex = np.ascontiguousarray(np.asarray([] if exclude is None else list(exclude), dtype=np.int64).reshape(-1))
        args = [h, _ptr(members)]
        if rank >= 2:
            args.append(_ptr(w) if w is not None else None)
        args += [k, _ptr(ex) if ex.size else None, int(ex.size)]
        if rank >= 1:
            args.append(ctypes.byref(flt) if flt is not None else None)
        if diverse:
            args += [ctypes.c_float(float(lam)), int(pool)]
        if capped:
            args.append(int(max_per_group))
        args += [int(topn), _ptr(idx), _ptr(score)]
        if diverse:
            args.append(_ptr(mmr))
        args.append(ctypes.byref(count))
        if capped:
            args.append(ctypes.byref(pool_rows))
        check(getattr(lib, f"{prefix}query_{'playlist' if members.dtype == np.int64 else 'mean'}_topn{level}")(*args))
    out = (idx[:count.value].copy(), score[:count.value].copy())
    if return_mmr:
        out += (mmr[:count.value].copy(),)
    if return_pool_rows:
        out += (pool_rows.value,)
    return out


def _request_ext(scales, rowset):
    """capi.RequestExt from checked scales (a float32 array or None) and rowset = (pointer, mode) or None.  (The arrays it points to
    are the caller's: they outlive the call.)"""
    return capi.RequestExt(ctypes.sizeof(capi.RequestExt), int(rowset[1]) if rowset is not None else 0,
                           _ptr(scales) if scales is not None else None,
                           rowset[0] if rowset is not None else None)


def _distance_request(lib, prefix: str, h, check, members, topn: int, exclude=None, where=None, labels=None, scales=None, rowset=None,
                      candidates=None):
    """One DISTANCE REQUEST (`prefix`query_distance_request): the `topn` rows nearest to the members by Euclidean distance.
    `members` is a (k, 12) float32 array (by value) or a 1-D int64 array of rows (never returned).  `exclude`, `where` and
    `labels` are the playlist request's.  Returns (ids, distances): nearest first, ties by row; for k > 1 a distance is the
    root-mean-square distance to the members.  `scales` (make_scales): FEATURE SCALES, through `prefix`query_distance_request_scaled.
    `rowset` = (pointer, mode): ROW SETS, through `prefix`query_distance_request_ext.  `candidates`: CANDIDATE LISTS, a sequence of
    global ids, through `prefix`query_distance_request_candidates."""
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    dist = np.empty(n_out, dtype=np.float32)
    count = ctypes.c_int(0)
    q = capi.DistanceQuery()
    keep = _fill_query(q, members, topn, exclude, where, labels)   # noqa: F841  (alive until the call has returned)
    res = capi.DistanceResult(_ptr(idx), _ptr(dist), ctypes.pointer(count))
    _call_request(lib, prefix, h, check, "distance", q, res, make_scales(scales) if scales is not None else None, rowset, candidates)
    return idx[:count.value].copy(), dist[:count.value].copy()


def _np_priors(priors) -> np.ndarray:
    """One prior per row (float32, contiguous); the library checks the values."""
    return np.ascontiguousarray(np.asarray(priors, dtype=np.float32).reshape(-1))


def _np_groups(groups) -> np.ndarray:
    """One group id per row (int32, contiguous): >= 0 a group, -1 ungrouped."""
    g = np.asarray(groups)
    if g.dtype.kind not in "iu" or (g.size and (g.min() < -(2 ** 31) or g.max() > 2 ** 31 - 1)):
        raise ValueError("groups must be integers that fit int32")
    return np.ascontiguousarray(g.astype(np.int32).reshape(-1))


def _np_members(queries) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(queries, dtype=np.float32).reshape(-1, capi.DIM))


def _np_rows(rows) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(list(rows), dtype=np.int64).reshape(-1))


class RowSet:
    """ROW SETS (include/mi355rec_diag.h): one bit per row of the engine it was made on (CosineEngine.row_set / NodeEngine.row_set),
    n / 8 bytes on the host and on every device copy.  Pass it as `seen=` (its rows are left out) or `only=` (only its rows are
    ranked).  It may grow (add); close() frees it, and the engine closes the sets it still has before it closes itself.  add or
    close while another thread runs a request with the set is the caller's error."""

    def __init__(self, owner, ids, create):
        self._lib = owner._lib
        self._owner = owner
        self._p = ctypes.c_void_p()
        a = _np_ids(ids)
        owner._set_check(create(owner._h, a.ctypes.data_as(ctypes.c_void_p) if a.size else None, int(a.size), ctypes.byref(self._p)))
        owner._sets.add(self)

    def _ptr(self):
        if not self._p:
            raise ValueError("this row set is closed")
        return self._p

    def add(self, ids) -> None:
        """Adds global ids (duplicates and ids already in the set are fine); a refused list leaves the set unchanged."""
        a = _np_ids(ids)
        rc = self._lib.mi355rec_rowset_add(self._ptr(), a.ctypes.data_as(ctypes.c_void_p) if a.size else None, int(a.size))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._lib.mi355rec_last_global_error() or b"").decode("utf-8", "replace"))

    @property
    def count(self) -> int:
        """The distinct rows of the engine in the set."""
        return int(self._lib.mi355rec_rowset_count(self._ptr()))

    def close(self) -> None:
        if getattr(self, "_p", None) is not None and self._p:
            self._lib.mi355rec_rowset_destroy(self._p)
            self._p = ctypes.c_void_p()
            self._owner._sets.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _np_ids(ids) -> np.ndarray:
    """Global ids of a row set (int64, contiguous); the library checks the values."""
    return np.ascontiguousarray(np.asarray([] if ids is None else ids, dtype=np.int64).reshape(-1))


class _RowSets:
    """What both engines share for ROW SETS: the sets they own, and `seen=` / `only=` resolved to (pointer, mode)."""

    @property
    def _sets(self):
        if "_row_sets" not in self.__dict__:
            self.__dict__["_row_sets"] = weakref.WeakSet()
        return self.__dict__["_row_sets"]

    def _close_sets(self) -> None:
        for s in list(self.__dict__.get("_row_sets", ())):
            s.close()

    def _with_set(self, seen, only, call):
        """call(rowset) with rowset = None, or (pointer, mode) of `seen` / `only`: a RowSet, or a plain id sequence, for which a
        temporary set is made and destroyed."""
        if seen is not None and only is not None:
            raise ValueError("seen= and only= are mutually exclusive: a request takes one row set")
        src, mode = (seen, capi.ROWSET_EXCLUDE) if seen is not None else (only, capi.ROWSET_ONLY)
        if src is None:
            return call(None)
        if isinstance(src, RowSet):
            return call((src._ptr(), mode))
        with self.row_set(src) as tmp:
            return call((tmp._ptr(), mode))


class _RequestFamily(_RowSets):
    """What both engines share for the playlist request family and the distance request: the calls that differ between a
    single handle and a node handle only in the C-ABI's symbol prefix (`_prefix`) and in how a return code is checked
    (`_check`).  Rows are local rows of a CosineEngine and global rows of a NodeEngine."""

    def _entry(self, name: str):
        return getattr(self._lib, self._prefix + name)

    def _set_per_row(self, name: str, values, convert) -> None:
        if values is None:
            self._check(self._entry(name)(self._h, None, 0))
            return
        a = convert(values)
        self._check(self._entry(name)(self._h, a.ctypes.data_as(ctypes.c_void_p), int(a.size)))

    # ---- LABELS (include/mi355rec_diag.h): label-filtered top-N ----
    def set_labels(self, labels) -> None:
        """One label per row in [0, capi.MAX_LABELS), -1 = unlabelled; None drops the labels."""
        self._set_per_row("set_labels", labels, _np_labels)

    # ---- PLAYLISTS (include/mi355rec_diag.h): top-N by the mean score against up to 32 songs ----
    def query_mean_topn(self, queries, topn: int, exclude=None, where=None, weights=None, labels=None, prior_weight=None,
                        scales=None, seen=None, only=None) -> Tuple[np.ndarray, np.ndarray]:
        """The best `topn` rows by the mean of their scores against the rows of `queries` (k x 12); `exclude`: global ids.
        `where`: {feature index or name: (lo, hi)}, only rows within every range are returned (FEATURE FILTERS; a
        filtered single query is k = 1); None calls the unfiltered entry point.
        `weights`: one signed float per member (WEIGHTED PLAYLISTS: score = sum w_k c_k / sum |w_k|, a negative weight is
        a dislike); None calls the entry point used without it.
        `scales`: FEATURE SCALES, 12 floats or {feature index or name: scale} (unnamed features 1.0): rows and members are
        multiplied feature by feature before the scores are taken (0 ignores a feature); not with prior_weight.
        `seen` / `only`: ROW SETS, a RowSet (row_set) or a plain sequence of global ids: the rows of `seen` are never returned (a
        listening history of any length); with `only`, only its rows are ranked (a candidate set).  Mutually exclusive.
        query_playlist_topn is the same for members given as rows of the engine; the members are then never returned
        (whatever their weight)."""
        return self._playlist(_np_members(queries), topn, exclude, where, weights, labels=labels, prior_weight=prior_weight, scales=scales,
                              seen=seen, only=only)

    def _playlist(self, members, topn, exclude, where, weights, level=None, labels=None, seen=None, only=None, candidates=None, **more):
        """Every playlist method's one way down.  `candidates`: CANDIDATE LISTS, passed by with_candidates' view alone."""
        return self._with_set(seen, only, lambda rowset: _playlist_family(
            self._lib, self._prefix, self._h, self._check, members, topn, exclude, where, weights, level, labels=labels,
            rowset=rowset, candidates=candidates, **more))

    # ---- DISTANCE REQUESTS (include/mi355rec_diag.h): the nearest rows by Euclidean distance ----
    def query_nearest(self, members, topn: int, exclude=None, where=None, labels=None) -> Tuple[np.ndarray, np.ndarray]:
        """The `topn` rows nearest to the rows of `members` (k x 12) by Euclidean distance over the 12 features: (ids,
        distances), nearest first.  k > 1: the root-mean-square distance to the members (as a ranking: the distance to their
        centroid).  `exclude`, `where`, `labels`: as in query_mean_topn."""
        return self._nearest(_np_members(members), topn, None, exclude, where, labels, None, None)

    def query_nearest_rows(self, rows, topn: int, exclude=None, where=None, labels=None) -> Tuple[np.ndarray, np.ndarray]:
        """The same for members given as rows of the engine; the members are never returned."""
        return self._nearest(_np_rows(rows), topn, None, exclude, where, labels, None, None)

    def query_nearest_scaled(self, members, topn: int, scales, exclude=None, where=None, labels=None, seen=None,
                             only=None) -> Tuple[np.ndarray, np.ndarray]:
        """query_nearest with FEATURE SCALES (`scales` as in query_mean_topn; None: none): the distances are taken between the
        scaled members and the scaled rows; the filter still tests the stored rows.  `seen` / `only`: ROW SETS, as in
        query_mean_topn (query_nearest itself keeps its parameter list)."""
        return self._nearest(_np_members(members), topn, scales, exclude, where, labels, seen, only)

    def query_nearest_rows_scaled(self, rows, topn: int, scales, exclude=None, where=None, labels=None, seen=None,
                                  only=None) -> Tuple[np.ndarray, np.ndarray]:
        """query_nearest_rows with FEATURE SCALES and ROW SETS."""
        return self._nearest(_np_rows(rows), topn, scales, exclude, where, labels, seen, only)

    def _nearest(self, members, topn, scales, exclude, where, labels, seen, only, candidates=None):
        return self._with_set(seen, only, lambda rowset: _distance_request(
            self._lib, self._prefix, self._h, self._check, members, topn, exclude, where, labels, scales, rowset, candidates))

    # ---- DIVERSIFIED TOP-N (include/mi355rec_diag.h): MMR picks from the top-`pool` of the weighted playlist call ----
    def query_mean_topn_diverse(self, queries, topn: int, lam, pool=None, exclude=None, where=None, weights=None, return_mmr=False,
                                labels=None, prior_weight=None, seen=None, only=None):
        """`topn` rows picked greedily from the `pool` most relevant (query_mean_topn's order): each pick maximises
        lam * relevance - (1 - lam) * (its largest similarity to a row already picked).  Pick order; scores = relevance.
        query_playlist_topn_diverse is the same for members given as rows of the engine (never returned)."""
        return self._playlist(_np_members(queries), topn, exclude, where, weights, "_diverse", lam=lam, pool=pool, return_mmr=return_mmr,
                              labels=labels, prior_weight=prior_weight, seen=seen, only=only)

    def set_groups(self, groups) -> None:
        """One group id per row (GROUP CAPS): >= 0 a group (an artist, say), -1 = never capped; None drops the groups."""
        self._set_per_row("set_groups", groups, _np_groups)

    def set_priors(self, priors) -> None:
        """One float per row in [-1, 1] (ROW PRIORS: popularity, freshness, a boost); None drops the priors."""
        self._set_per_row("set_priors", priors, _np_priors)

    def query_mean_topn_capped(self, queries, topn: int, max_per_group: int, lam=1.0, pool=None, exclude=None, where=None,
                               weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None,
                               seen=None, only=None):
        """query_mean_topn_diverse with at most `max_per_group` results per group of set_groups (GROUP CAPS);
        query_playlist_topn_capped: for members given as rows of the engine."""
        return self._playlist(_np_members(queries), topn, exclude, where, weights, "_capped", lam=lam, pool=pool,
                              max_per_group=max_per_group, return_mmr=return_mmr, return_pool_rows=return_pool_rows,
                              labels=labels, prior_weight=prior_weight, seen=seen, only=only)


class _Listed:
    """An engine seen through a CANDIDATE LIST (with_candidates): the engine's request-family methods, each ranking within the list.
    A method of the engine's class runs with THIS object as its self, so its one call down (self._playlist / self._nearest) lands
    here and goes on to the engine's with the list as an explicit argument.  The engine itself is never written to."""

    def __init__(self, eng, candidates):
        self._eng, self._ids = eng, _np_ids(candidates)

    def __getattr__(self, name):
        if not (name.startswith("query_mean_topn") or name.startswith("query_playlist_topn") or name.startswith("query_nearest")):
            raise AttributeError(f"{name}: a candidate list goes with query_mean_topn*, query_playlist_topn* and query_nearest*")
        return types.MethodType(getattr(type(self._eng), name), self)

    def _playlist(self, *args, **kwargs):
        return self._eng._playlist(*args, candidates=self._ids, **kwargs)

    def _nearest(self, *args, **kwargs):
        return self._eng._nearest(*args, candidates=self._ids, **kwargs)


def with_candidates(eng, candidates):
    """CANDIDATE LISTS (include/mi355rec_diag.h): `eng` (a CosineEngine, a lane or a NodeEngine) restricted to `candidates`, a plain
    sequence or an int64 array of global ids in any order (duplicates fine, up to capi.MAX_CANDIDATES; empty: nothing is returned).
    The object returned has the engine's query_mean_topn*, query_playlist_topn* and query_nearest* methods with their own
    parameters; each gathers and ranks ONLY the listed rows, where an `only=` row set would make a pass over the whole catalogue.
    It composes with every other argument: with `seen=` the answer lies in the list minus the set (candidates minus a listening
    history), with `only=` in both.  The result is bit for bit that of `only=candidates`.
        ids, scores = with_candidates(eng, first_stage_ids).query_playlist_topn(playlist_rows, 100, seen=history)
    (The engines' own methods keep their parameter lists: tests/test_engine_surface.py records them.)"""
    return _Listed(eng, candidates)


def candidate_scores(eng, candidates, *, queries=None, rows=None, metric="cosine", exclude=None, where=None, weights=None, labels=None,
                     prior_weight=None, scales=None, seen=None, only=None) -> Tuple[np.ndarray, np.ndarray]:
    """CANDIDATE SCORES (include/mi355rec_diag.h): what the request is worth at EVERY listed row, in list order, for a blender that
    mixes a first stage's score with the engine's.  `eng`: a CosineEngine, a lane or a NodeEngine; `candidates`: global ids, any
    order, duplicates fine, up to capi.MAX_CANDIDATES.  The request is given as to query_mean_topn / query_playlist_topn
    (metric="cosine": `queries` k x 12 by value or `rows` of the engine; `weights`, `prior_weight`) or to query_nearest*
    (metric="distance"), with `exclude`, `where`, `labels`, `scales`, `seen` / `only` as there.
    Returns (values float32[n], admissible bool[n]): values[i] is bit for bit the score (the distance) the same request's top-N call
    reports for candidates[i]; where candidates[i] can never be returned (excluded, a member given by row, rejected by the row set,
    the label set or the filter, a distance that is not finite, an id outside a single handle's rows) it is NaN and the flag is False."""
    if (queries is None) == (rows is None):
        raise ValueError("candidate_scores takes queries= (members by value) or rows= (members by row), one of them")
    if metric not in ("cosine", "distance"):
        raise ValueError(f"metric {metric!r}: 'cosine' or 'distance'")
    dist = metric == "distance"
    if dist and (weights is not None or prior_weight is not None):
        raise ValueError("a distance request takes no weights and no prior_weight")
    members = _np_members(queries) if queries is not None else _np_rows(rows)
    k = int(members.shape[0])
    cand = _np_ids(candidates)
    values = np.empty(cand.size, dtype=np.float32)
    flags = np.empty(cand.size, dtype=np.uint8)
    q = capi.DistanceQuery() if dist else capi.PlaylistQuery()
    keep = _fill_query(q, members, 1, exclude, where, labels)   # noqa: F841  (topn is checked and otherwise unused)
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if w.size != k:
            raise ValueError(f"{w.size} weights for {k} songs: one weight per song")
        q.weights = _ptr(w)
    if prior_weight is not None:
        q.flags |= capi.PQ_PRIOR
        q.prior_weight = float(prior_weight)
    a = make_scales(scales) if scales is not None else None
    entry = getattr(eng._lib, f"{eng._prefix}score_{'distance' if dist else 'playlist'}_request_candidates")

    def call(rowset):
        ext = _request_ext(a, rowset)
        eng._check(entry(eng._h, ctypes.byref(q), ctypes.byref(ext), _ptr(cand) if cand.size else None, int(cand.size),
                         _ptr(values) if cand.size else None, _ptr(flags) if cand.size else None))

    eng._with_set(seen, only, call)
    return values, flags.astype(bool)


def query_anyof(eng, topn, members=None, rows=None, exclude=None, where=None, labels=None, seen=None, only=None):
    """ANY-OF REQUESTS (include/mi355rec_diag.h): the `topn` rows by their BEST cosine among the members ("like any of these"), and
    which member each matched.  `eng`: a CosineEngine, a lane or a NodeEngine; `members` k x 12 by value or `rows` of the engine (never
    returned), one of them; `exclude`, `where`, `labels`, `seen` / `only` as in query_playlist_topn.
    Returns (ids int64[c], scores float32[c], member int32[c]): member[i] is the smallest index into the member list whose cosine
    with row ids[i] is scores[i].
        ids, scores, member = query_anyof(eng, 100, rows=playlist_rows, seen=history)
    (The engines' own methods keep their parameter lists: tests/test_engine_surface.py records them.)"""
    if (members is None) == (rows is None):
        raise ValueError("query_anyof takes members= (by value) or rows= (by row), one of them")
    m = _np_members(members) if members is not None else _np_rows(rows)
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    score = np.empty(n_out, dtype=np.float32)
    member = np.empty(n_out, dtype=np.int32)
    count = ctypes.c_int(0)
    q = capi.AnyOfQuery()
    keep = _fill_query(q, m, topn, exclude, where, labels)   # noqa: F841  (alive until the call has returned)
    res = capi.AnyOfResult(_ptr(idx), _ptr(score), _ptr(member), ctypes.pointer(count))
    eng._with_set(seen, only, lambda rowset: _call_request(eng._lib, eng._prefix, eng._h, eng._check, "anyof", q, res, rowset=rowset))
    c = count.value
    return idx[:c].copy(), score[:c].copy(), member[:c].copy()


def query_manhattan(eng, topn, members=None, rows=None, exclude=None, where=None, labels=None, seen=None, only=None):
    """MANHATTAN REQUESTS (include/mi355rec_diag.h): the `topn` rows NEAREST by L1 distance to the members (the mean over the
    members of sum_j |q_kj - x_j|).  `eng`: a CosineEngine, a lane or a NodeEngine; `members` k x 12 by value or `rows` of the
    engine (never returned), one of them; `exclude`, `where`, `labels`, `seen` / `only` as in query_playlist_topn.
    Returns (ids int64[c], distances float32[c]), nearest first, ties by id.
        ids, distances = query_manhattan(eng, 100, rows=playlist_rows, seen=history)
    (The engines' own methods keep their parameter lists: tests/test_engine_surface.py records them.)"""
    if (members is None) == (rows is None):
        raise ValueError("query_manhattan takes members= (by value) or rows= (by row), one of them")
    m = _np_members(members) if members is not None else _np_rows(rows)
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    dist = np.empty(n_out, dtype=np.float32)
    count = ctypes.c_int(0)
    q = capi.ManhattanQuery()
    keep = _fill_query(q, m, topn, exclude, where, labels)   # noqa: F841  (alive until the call has returned)
    res = capi.ManhattanResult(_ptr(idx), _ptr(dist), ctypes.pointer(count))
    eng._with_set(seen, only, lambda rowset: _call_request(eng._lib, eng._prefix, eng._h, eng._check, "manhattan", q, res, rowset=rowset))
    c = count.value
    return idx[:c].copy(), dist[:c].copy()


def query_jaccard(eng, topn, members=None, rows=None, exclude=None, where=None, labels=None, seen=None, only=None):
    """JACCARD REQUESTS (include/mi355rec_diag.h): the `topn` rows most similar to the members by weighted (Ruzicka) Jaccard
    similarity (the mean over the members of sum_j min(q_kj, x_j) / sum_j max(q_kj, x_j)).  `eng`: a CosineEngine, a lane or a
    NodeEngine; `members` k x 12 by value or `rows` of the engine (never returned), one of them; `exclude`, `where`, `labels`,
    `seen` / `only` as in query_playlist_topn.
    Returns (ids int64[c], similarities float32[c]), most similar first, ties by id.
        ids, similarities = query_jaccard(eng, 100, rows=playlist_rows, seen=history)
    (The engines' own methods keep their parameter lists: tests/test_engine_surface.py records them.)"""
    if (members is None) == (rows is None):
        raise ValueError("query_jaccard takes members= (by value) or rows= (by row), one of them")
    m = _np_members(members) if members is not None else _np_rows(rows)
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    sim = np.empty(n_out, dtype=np.float32)
    count = ctypes.c_int(0)
    q = capi.JaccardQuery()
    keep = _fill_query(q, m, topn, exclude, where, labels)   # noqa: F841  (alive until the call has returned)
    res = capi.JaccardResult(_ptr(idx), _ptr(sim), ctypes.pointer(count))
    eng._with_set(seen, only, lambda rowset: _call_request(eng._lib, eng._prefix, eng._h, eng._check, "jaccard", q, res, rowset=rowset))
    c = count.value
    return idx[:c].copy(), sim[:c].copy()


def query_bounded(eng, topn, bound, metric="cosine", members=None, rows=None, exclude=None, where=None, labels=None, seen=None, only=None):
    """BOUNDED REQUESTS (include/mi355rec_diag.h): only the rows that are good enough, and how many there are.  metric="cosine":
    the rows whose unweighted mean cosine to the members is >= `bound`; metric="euclidean": the rows whose distance (what
    query_nearest reports) is <= the radius `bound`.  `eng`: a CosineEngine, a lane or a NodeEngine; `members` k x 12 by value or
    `rows` of the engine (never returned, never counted), one of them; `exclude`, `where`, `labels`, `seen` / `only` as in
    query_playlist_topn.  `topn` may be 0: count only.
    Returns (ids int64[c], scores float32[c], total): the leading c = min(topn, total) matching rows, best first (for the Euclidean
    metric `scores` holds distances, nearest first), and the exact number of matching rows.
        ids, scores, total = query_bounded(eng, 100, 0.9, rows=playlist_rows, seen=history)
    (The engines' own methods keep their parameter lists: tests/test_engine_surface.py records them.)"""
    if (members is None) == (rows is None):
        raise ValueError("query_bounded takes members= (by value) or rows= (by row), one of them")
    if metric not in ("cosine", "euclidean"):
        raise ValueError(f"metric {metric!r}: 'cosine' or 'euclidean'")
    m = _np_members(members) if members is not None else _np_rows(rows)
    n_out = max(int(topn), 1)
    idx = np.empty(n_out, dtype=np.int64)
    score = np.empty(n_out, dtype=np.float32)
    count = ctypes.c_int(0)
    total = ctypes.c_int64(0)
    q = capi.BoundedQuery()
    keep = _fill_query(q, m, topn, exclude, where, labels)   # noqa: F841  (alive until the call has returned)
    q.metric = capi.BOUNDED_EUCLIDEAN if metric == "euclidean" else capi.BOUNDED_COSINE
    q.bound = float(bound)
    res = capi.BoundedResult(_ptr(idx), _ptr(score), ctypes.pointer(count), ctypes.pointer(total))
    eng._with_set(seen, only, lambda rowset: _call_request(eng._lib, eng._prefix, eng._h, eng._check, "bounded", q, res, rowset=rowset))
    c = count.value
    return idx[:c].copy(), score[:c].copy(), int(total.value)


def candidates_counters(eng) -> dict:
    """mi355rec_candidates_counters of a CosineEngine (or a lane): the requests that took the gather launch and the distinct
    in-shard list entries those launches were given, since the handle was created."""
    q, r = ctypes.c_int64(0), ctypes.c_int64(0)
    capi.check(eng._lib.mi355rec_candidates_counters(eng._h, ctypes.byref(q), ctypes.byref(r)), eng._h)
    return {"requests": q.value, "rows_gathered": r.value}


class CosineEngine(_RequestFamily):
    """One row shard of the N x 12 fp32 catalogue resident on one MI355X.

    Replaces the reference's device state (d_features / d_queryFeature /
    d_similarities, Recommender.h:91-94) and its per-query pipeline
    (Recommender.cu:184-254 + :293-315).
    """

    _prefix = "mi355rec_"

    def __init__(self, feats, device: int = 0, row_base: int = 0, flags: int = 0):
        """flags: capi.CREATE_NO_REPLICA = keep the fp32 rows only (48 B per row resident instead of 84)."""
        self._lib = capi.lib()
        self._h = ctypes.c_void_p()
        self._keepalive = None
        self.device = int(device)
        try:
            import torch
        except Exception:  # pragma: no cover - torch is part of the image
            torch = None
        if torch is not None and isinstance(feats, torch.Tensor):
            if not feats.is_cuda:
                feats = feats.numpy()
            else:
                if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != capi.DIM:
                    raise ValueError("catalogue must be float32 [n, 12]")
                if not feats.is_contiguous():
                    raise ValueError("catalogue tensor must be contiguous (row-major)")
                self._keepalive = feats
                self.device = feats.device.index if feats.device.index is not None else 0
                rc = self._lib.mi355rec_create_device_ex(
                    ctypes.c_void_p(feats.data_ptr()), feats.shape[0], feats.shape[1],
                    self.device, int(row_base), int(flags), ctypes.byref(self._h))
                capi.check(rc)
                self.rows = int(feats.shape[0])
                self.row_base = int(row_base)
                return
        arr = _np_f32(feats)
        if arr.ndim != 2 or arr.shape[1] != capi.DIM:
            raise ValueError("catalogue must be float32 [n, 12]")
        rc = self._lib.mi355rec_create_ex(
            arr.ctypes.data_as(ctypes.c_void_p), arr.shape[0], arr.shape[1], self.device,
            int(row_base), int(flags), ctypes.byref(self._h))
        capi.check(rc)
        self.rows = int(arr.shape[0])
        self.row_base = int(row_base)

    def lane(self) -> "CosineEngine":
        """Another handle over the same rows and replicas with its own stream state (mi355rec_create_lane): queries dealt
        alternately over two lanes on two streams overlap where one handle's launches cannot."""
        other = CosineEngine.__new__(CosineEngine)
        other._lib = self._lib
        other._h = ctypes.c_void_p()
        other._keepalive = self._keepalive
        other.device = self.device
        other.rows = self.rows
        other.row_base = self.row_base
        capi.check(self._lib.mi355rec_create_lane(self._h, ctypes.byref(other._h)), self._h)
        return other

    def lane_status(self) -> dict:
        """What mi355rec_create_lane found for this lane's stream: {"stream_attempts", "overlaps_parent" (1 / 0 / -1)}."""
        a, o = ctypes.c_int(0), ctypes.c_int(-1)
        capi.check(self._lib.mi355rec_lane_status(self._h, ctypes.byref(a), ctypes.byref(o)), self._h)
        return {"stream_attempts": a.value, "overlaps_parent": o.value}

    def own_stream(self):
        """The HIP stream the library created with this handle, as a torch stream (mi355rec_own_stream): the stream to run a
        lane on — streams taken from torch's pool later may share a hardware queue, and then lanes do not overlap."""
        import torch
        return torch.cuda.ExternalStream(int(self._lib.mi355rec_own_stream(self._h)), device=self.device)

    # -- lifetime ---------------------------------------------------------
    def row_set(self, ids) -> RowSet:
        """A ROW SET of this handle from global ids (0 <= id < 2**32; ids of other shards match nothing), usable on this engine
        and its lanes as `seen=` or `only=`."""
        return RowSet(self, ids, self._lib.mi355rec_rowset_create)

    def _check(self, rc: int) -> None:
        capi.check(rc, self._h)

    _set_check = _check

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._close_sets()
            self._lib.mi355rec_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- synchronous host API ------------------------------------------------
    def scores_row(self, local_row: int) -> np.ndarray:
        out = np.empty(self.rows, dtype=np.float32)
        capi.check(self._lib.mi355rec_scores_row(self._h, int(local_row), out.ctypes.data_as(ctypes.c_void_p)), self._h)
        return out

    def scores(self, query) -> np.ndarray:
        q = _np_f32(query).reshape(capi.DIM)
        out = np.empty(self.rows, dtype=np.float32)
        capi.check(self._lib.mi355rec_scores(self._h, q.ctypes.data_as(ctypes.c_void_p),
                                             out.ctypes.data_as(ctypes.c_void_p)), self._h)
        return out

    def query_row_topn(self, local_row: int, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        n_out = max(int(topn), 1)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        capi.check(self._lib.mi355rec_query_row_topn(
            self._h, int(local_row), int(topn), idx.ctypes.data_as(ctypes.c_void_p),
            score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)), self._h)
        return idx[:count.value].copy(), score[:count.value].copy()

    def bound_query_row_topn(self, topn: int):
        """`mi355rec_query_row_topn` with CALLER-OWNED result buffers bound once, as a C or C++ host would call it: returns
        call(row) -> (idx, score, count), the same two arrays every time (valid until the next call).  What a latency
        loop should use: query_row_topn() allocates and converts per call (~3 us of Python around a 46 us query)."""
        topn = int(topn)
        n_out = max(topn, 1)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        p_idx, p_score, p_count = idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)
        fn, h = self._lib.mi355rec_query_row_topn, self._h

        def call(local_row: int):
            rc = fn(h, local_row, topn, p_idx, p_score, p_count)
            if rc:
                capi.check(rc, h)
            return idx, score, count.value
        return call

    def query_topn(self, query, exclude_global: int, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _np_f32(query).reshape(capi.DIM)
        n_out = max(int(topn), 1)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        capi.check(self._lib.mi355rec_query_topn(
            self._h, q.ctypes.data_as(ctypes.c_void_p), int(exclude_global), int(topn),
            idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p),
            ctypes.byref(count)), self._h)
        return idx[:count.value].copy(), score[:count.value].copy()

    def query_batch_topn(self, queries, exclude_global, topn: int):
        q = _np_f32(queries).reshape(-1, capi.DIM)
        b = q.shape[0]
        excl = None
        if exclude_global is not None:
            excl = np.ascontiguousarray(np.asarray(exclude_global, dtype=np.int64).reshape(b))
        n_out = max(int(topn), 1)
        idx = np.empty((b, n_out), dtype=np.int64)
        score = np.empty((b, n_out), dtype=np.float32)
        counts = np.zeros(b, dtype=np.int32)
        capi.check(self._lib.mi355rec_query_batch_topn(
            self._h, q.ctypes.data_as(ctypes.c_void_p), b,
            excl.ctypes.data_as(ctypes.c_void_p) if excl is not None else None, int(topn),
            idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p),
            counts.ctypes.data_as(ctypes.c_void_p)), self._h)
        return idx, score, counts

    # -- asynchronous device API -------------------------------------------
    @staticmethod
    def _stream_ptr(stream) -> ctypes.c_void_p:
        if stream is None:
            import torch
            stream = torch.cuda.current_stream()
        if hasattr(stream, "cuda_stream"):
            return ctypes.c_void_p(stream.cuda_stream)
        return ctypes.c_void_p(int(stream))

    def enqueue_row_keys(self, local_row: int, topn: int, out_keys, stream=None) -> None:
        capi.check(self._lib.mi355rec_enqueue_row_keys(
            self._h, int(local_row), int(topn), ctypes.c_void_p(out_keys.data_ptr()),
            self._stream_ptr(stream)), self._h)

    def enqueue_query_keys(self, query, exclude_global: int, topn: int, out_keys, stream=None) -> None:
        q = _np_f32(query).reshape(capi.DIM)
        capi.check(self._lib.mi355rec_enqueue_query_keys(
            self._h, q.ctypes.data_as(ctypes.c_void_p), int(exclude_global), int(topn),
            ctypes.c_void_p(out_keys.data_ptr()), self._stream_ptr(stream)), self._h)

    def enqueue_row_keys_streamed(self, local_row: int, topn: int, out_keys, stream=None) -> None:
        """Deferred merge: complete after the NEXT streamed call's work, or after enqueue_flush."""
        capi.check(self._lib.mi355rec_enqueue_row_keys_streamed(
            self._h, int(local_row), int(topn), ctypes.c_void_p(out_keys.data_ptr()),
            self._stream_ptr(stream)), self._h)

    def bound_enqueue_row_keys_streamed(self, topn: int, stream=None):
        """`mi355rec_enqueue_row_keys_streamed` with everything but the row and the output pointer bound once, as a C or C++
        host would call it: returns call(row, out_ptr) with out_ptr = ctypes.c_void_p(tensor.data_ptr()).  What a
        throughput loop should use: the general wrapper spends ~2 us per call on attribute look-ups around an 8 us launch,
        and a two-lane stream at 17 us per query notices (tools/lanes.cpp: 16.7 us from C++)."""
        fn, h, sp, topn = self._lib.mi355rec_enqueue_row_keys_streamed, self._h, self._stream_ptr(stream), int(topn)

        def call(row: int, out_ptr) -> None:
            rc = fn(h, row, topn, out_ptr, sp)
            if rc:
                capi.check(rc, h)
        return call

    def enqueue_query_keys_streamed(self, query, exclude_global: int, topn: int, out_keys, stream=None) -> None:
        q = _np_f32(query).reshape(capi.DIM)
        capi.check(self._lib.mi355rec_enqueue_query_keys_streamed(
            self._h, q.ctypes.data_as(ctypes.c_void_p), int(exclude_global), int(topn),
            ctypes.c_void_p(out_keys.data_ptr()), self._stream_ptr(stream)), self._h)

    def enqueue_flush(self, stream=None) -> None:
        capi.check(self._lib.mi355rec_enqueue_flush(self._h, self._stream_ptr(stream)), self._h)

    def enqueue_batch_keys(self, queries, exclude_global, topn: int, out_keys, stream=None) -> None:
        """Multi-query passes: 12 queries share one scan of the shard (topn <= 128)."""
        q = _np_f32(queries).reshape(-1, capi.DIM)
        excl = None
        if exclude_global is not None:
            excl = np.ascontiguousarray(np.asarray(exclude_global, dtype=np.int64).reshape(q.shape[0]))
        capi.check(self._lib.mi355rec_enqueue_batch_keys(
            self._h, q.ctypes.data_as(ctypes.c_void_p),
            excl.ctypes.data_as(ctypes.c_void_p) if excl is not None else None, q.shape[0], int(topn),
            ctypes.c_void_p(out_keys.data_ptr()), self._stream_ptr(stream)), self._h)

    def enqueue_batch_keys_streamed(self, queries, exclude_global, topn: int, out_keys, stream=None) -> None:
        """A stream of batches: complete after the second streamed batch call behind it, or after enqueue_flush."""
        q = _np_f32(queries).reshape(-1, capi.DIM)
        excl = None
        if exclude_global is not None:
            excl = np.ascontiguousarray(np.asarray(exclude_global, dtype=np.int64).reshape(q.shape[0]))
        capi.check(self._lib.mi355rec_enqueue_batch_keys_streamed(
            self._h, q.ctypes.data_as(ctypes.c_void_p),
            excl.ctypes.data_as(ctypes.c_void_p) if excl is not None else None, q.shape[0], int(topn),
            ctypes.c_void_p(out_keys.data_ptr()), self._stream_ptr(stream)), self._h)

    def enqueue_batch_keys_dev(self, queries_dev, exclude_dev, topn: int, out_keys, stream=None) -> None:
        """Batched matrix-core path over queries already in device memory
        (float32 [batch, 12] tensor; exclude_dev int64 [batch] tensor or None)."""
        capi.check(self._lib.mi355rec_enqueue_batch_keys_dev(
            self._h, ctypes.c_void_p(queries_dev.data_ptr()),
            ctypes.c_void_p(exclude_dev.data_ptr()) if exclude_dev is not None else None,
            int(queries_dev.shape[0]), int(topn), ctypes.c_void_p(out_keys.data_ptr()),
            self._stream_ptr(stream)), self._h)

    def batched_last_counters(self) -> dict:
        """Diagnostics of the last chunk served by the batched path (synchronises)."""
        sp, qd, mx = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        tot = ctypes.c_int64(0)
        capi.check(self._lib.mi355rec_batched_last_counters(
            self._h, ctypes.byref(sp), ctypes.byref(qd), ctypes.byref(tot), ctypes.byref(mx)), self._h)
        return {"special_rows": sp.value, "queued_queries": qd.value, "candidates_total": tot.value,
                "candidates_max": mx.value}

    def batched_pass2_pairs(self) -> dict:
        """(tile, query block) pairs pass 2 of the last batched chunk ran its MFMAs for, out of all (synchronises)."""
        done, total = ctypes.c_int64(0), ctypes.c_int64(0)
        capi.check(self._lib.mi355rec_batched_pass2_pairs(self._h, ctypes.byref(done), ctypes.byref(total)), self._h)
        return {"pairs_done": int(done.value), "pairs_total": int(total.value)}

    def set_replica(self, mode: int) -> None:
        """capi.REPLICA_AUTO / REPLICA_OFF (fp32 rows only) / REPLICA_ON: which copy single queries scan."""
        capi.check(self._lib.mi355rec_set_replica(self._h, int(mode)), self._h)

    def replica_counters(self) -> dict:
        """Cumulative: scans over the replica and rows they sent to the exact fp32 chain (synchronises)."""
        scans, rows = ctypes.c_int64(0), ctypes.c_int64(0)
        capi.check(self._lib.mi355rec_replica_counters(self._h, ctypes.byref(scans), ctypes.byref(rows)), self._h)
        return {"scans": int(scans.value), "rescored_rows": int(rows.value)}

    def set_sample(self, mode: int) -> None:
        """capi.SAMPLE_AUTO / SAMPLE_STRIDED / SAMPLE_BUCKETED: which cutoff sample single queries over the 8-bit replica take."""
        capi.check(self._lib.mi355rec_set_sample(self._h, int(mode)), self._h)

    def bucket_sample_info(self) -> dict:
        """The bucketed sample of the handle (base_rows 0: it has none), the mode set and what the last query took."""
        info = capi.BucketSampleInfo()
        capi.check(self._lib.mi355rec_bucket_sample_info(self._h, ctypes.byref(info)), self._h)
        return {name: getattr(info, name) for name, _ in info._fields_}

    def bucket_sample_rows(self):
        """(sample_rows int32[regions * 2048], region_tab int32[regions, 2]) copied to the host."""
        info = self.bucket_sample_info()
        rows = np.empty(info["regions"] * 2048, dtype=np.int32)
        tab = np.empty((info["regions"], 2), dtype=np.int32)
        capi.check(self._lib.mi355rec_bucket_sample_rows(self._h, rows.ctypes.data_as(ctypes.c_void_p),
                                                         tab.ctypes.data_as(ctypes.c_void_p)), self._h)
        return rows, tab

    def debug_handoff(self, flags: int) -> None:
        """Test hook (capi.DEBUG_HANDOFF_*): poison / drop the cross-workgroup hand-offs of the streamed scans."""
        capi.check(self._lib.mi355rec_debug_handoff(self._h, int(flags)), self._h)

    def rebuild_replica(self) -> None:
        """After overwriting a borrowed catalogue in place (synchronous)."""
        capi.check(self._lib.mi355rec_rebuild_replica(self._h), self._h)

    # -- ROW UPDATES ------------------------------------------------------------
    def update_rows(self, local_rows, feats=None) -> None:
        """Rows change in place (mi355rec_update_rows): afterwards every route of this handle and of its lanes answers as a handle
        freshly created from the updated matrix would.  local_rows: distinct rows of this handle; feats: [len(local_rows), 12]
        float32, or None when the caller has already written those rows of the torch tensor the engine was created over.
        Over such a tensor, feats is written into the tensor here (the engine borrows it), then the derived data is redone; the
        library is asked first, so a refused update leaves the tensor as it was (update_info counts that path as two calls).
        Flush every lane first (enqueue_flush) and let no other thread use the group meanwhile."""
        rows = np.ascontiguousarray(np.asarray(local_rows, dtype=np.int64).reshape(-1))
        rows_p = rows.ctypes.data_as(ctypes.c_void_p) if rows.size else None
        if feats is not None:
            arr = _np_f32(feats.detach().cpu().numpy() if hasattr(feats, "detach") else feats).reshape(-1, capi.DIM)
            if arr.shape[0] != rows.size:
                raise ValueError(f"{arr.shape[0]} feature rows for {rows.size} row ids")
            if self._keepalive is None:
                capi.check(self._lib.mi355rec_update_rows(self._h, rows_p, rows.size, arr.ctypes.data_as(ctypes.c_void_p)), self._h)
                return
            # The library is asked FIRST, with NULL rows and the tensor as it is (in effect a no-op: it redoes the entries of
            # unchanged rows): whatever it refuses (a row out of range or named twice, another lane with a streamed query open) is
            # refused before the tensor is written.
            import torch
            t = self._keepalive
            torch.cuda.synchronize(t.device)
            capi.check(self._lib.mi355rec_update_rows(self._h, rows_p, rows.size, None), self._h)
            t[torch.from_numpy(rows).to(t.device)] = torch.from_numpy(arr).to(t.device)
        if self._keepalive is not None:
            import torch
            torch.cuda.synchronize(self._keepalive.device)   # the tensor's writes are done before the library reads the rows
        capi.check(self._lib.mi355rec_update_rows(self._h, rows_p, rows.size, None), self._h)

    def update_info(self) -> dict:
        """{"calls", "rows", "rows_since_snapshot", "last_ms"} (mi355rec_update_info): rows_since_snapshot is the cue for an eventual
        rebuild_replica, which refreshes the bucketed sample and the anchor tables and resets it."""
        info = capi.UpdateInfo()
        info.size = ctypes.sizeof(capi.UpdateInfo)
        capi.check(self._lib.mi355rec_update_info(self._h, ctypes.byref(info)), self._h)
        return {"calls": info.calls, "rows": info.rows, "rows_since_snapshot": info.rows_since_snapshot, "last_ms": info.last_ms}

    def replica_entries(self, local_rows):
        """The stored replica entries of the given rows (mi355rec_replica_entries): (fp16 [k, 24] uint8, 8-bit [k, 12] uint8,
        norms [k] float32 — NaN-filled where the handle has built no norms).  For tests: an updated handle against a fresh one."""
        rows = np.ascontiguousarray(np.asarray(local_rows, dtype=np.int64).reshape(-1))
        half = np.zeros((rows.size, 24), dtype=np.uint8)
        q8 = np.zeros((rows.size, 12), dtype=np.uint8)
        norms = np.full(rows.size, np.nan, dtype=np.float32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        capi.check(self._lib.mi355rec_replica_entries(self._h, ptr(rows), rows.size, ptr(half), ptr(q8), ptr(norms)), self._h)
        return half, q8, norms

    def set_batch_path(self, path: int) -> None:
        """capi.BATCH_AUTO / BATCH_MULTI / BATCH_MFMA (tests, A/B measurements)."""
        capi.check(self._lib.mi355rec_set_batch_path(self._h, int(path)), self._h)

    def enqueue_merge_keys(self, lists, n_lists: int, list_len: int, topn: int, out_keys,
                           out_idx=None, out_score=None, stream=None) -> None:
        capi.check(self._lib.mi355rec_enqueue_merge_keys(
            self._h, ctypes.c_void_p(lists.data_ptr()), int(n_lists), int(list_len), int(topn),
            ctypes.c_void_p(out_keys.data_ptr()),
            ctypes.c_void_p(out_idx.data_ptr()) if out_idx is not None else None,
            ctypes.c_void_p(out_score.data_ptr()) if out_score is not None else None,
            self._stream_ptr(stream)), self._h)

    def enqueue_merge_keys_batch(self, lists, n_lists: int, list_len: int, list_stride: int, query_stride: int,
                                 batch: int, topn: int, out_keys, out_idx=None, out_score=None, stream=None) -> None:
        capi.check(self._lib.mi355rec_enqueue_merge_keys_batch(
            self._h, ctypes.c_void_p(lists.data_ptr()), int(n_lists), int(list_len), int(list_stride),
            int(query_stride), int(batch), int(topn), ctypes.c_void_p(out_keys.data_ptr()),
            ctypes.c_void_p(out_idx.data_ptr()) if out_idx is not None else None,
            ctypes.c_void_p(out_score.data_ptr()) if out_score is not None else None,
            self._stream_ptr(stream)), self._h)

    def enqueue_scores(self, local_row: int, query, out_scores, stream=None) -> None:
        q = None if query is None else _np_f32(query).reshape(capi.DIM)
        capi.check(self._lib.mi355rec_enqueue_scores(
            self._h, int(local_row), q.ctypes.data_as(ctypes.c_void_p) if q is not None else None,
            ctypes.c_void_p(out_scores.data_ptr()), self._stream_ptr(stream)), self._h)

    def enqueue_stream_probe(self, sink, stream=None, which: int = capi.PROBE_FP32_ROWS) -> None:
        """The plain read-only stream over one of the handle's buffers (fp32 rows, fp16 replica, 8-bit replica)."""
        capi.check(self._lib.mi355rec_enqueue_stream_probe_of(
            self._h, int(which), ctypes.c_void_p(sink.data_ptr()), self._stream_ptr(stream)), self._h)

    def set_timing(self, enabled) -> None:
        """0/False off, 1/True every launch, k > 1 every k-th launch."""
        capi.check(self._lib.mi355rec_set_timing(self._h, int(enabled)), self._h)

    def stats(self) -> capi.Stats:
        st = capi.Stats()
        capi.check(self._lib.mi355rec_stats(self._h, ctypes.byref(st)), self._h)
        return st

    # ---- LABELS (include/mi355rec_diag.h): label-filtered top-N ----
    def query_row_topn_labels(self, local_row: int, labels, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        """The best `topn` rows whose label is in `labels`, the query row excluded."""
        return _labels_query(self._lib.mi355rec_query_row_topn_labels, self._h, lambda rc: capi.check(rc, self._h),
                             (int(local_row),), labels, topn)

    def query_topn_labels(self, query, exclude_global: int, labels, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _np_f32(query).reshape(capi.DIM)
        return _labels_query(self._lib.mi355rec_query_topn_labels, self._h, lambda rc: capi.check(rc, self._h),
                             (q.ctypes.data_as(ctypes.c_void_p), int(exclude_global)), labels, topn)

    def label_counters(self) -> dict:
        q, r = ctypes.c_int64(0), ctypes.c_int64(0)
        capi.check(self._lib.mi355rec_label_counters(self._h, ctypes.byref(q), ctypes.byref(r)), self._h)
        return {"queries": q.value, "rows_scanned": r.value}


    # ---- the by-row forms of the request family (_RequestFamily): the members are rows of this handle ----
    def query_playlist_topn(self, local_rows, topn: int, exclude=None, where=None, weights=None, labels=None, prior_weight=None,
                            scales=None, seen=None, only=None) -> Tuple[np.ndarray, np.ndarray]:
        """The same for members given as rows of this handle; the members are never returned (whatever their weight)."""
        return self._playlist(_np_rows(local_rows), topn, exclude, where, weights, labels=labels, prior_weight=prior_weight, scales=scales,
                              seen=seen, only=only)

    def query_playlist_topn_diverse(self, local_rows, topn: int, lam, pool=None, exclude=None, where=None, weights=None,
                                    return_mmr=False, labels=None, prior_weight=None, seen=None, only=None):
        """The same for members given as rows of this handle (never returned)."""
        return self._playlist(_np_rows(local_rows), topn, exclude, where, weights, "_diverse", lam=lam, pool=pool, return_mmr=return_mmr,
                              labels=labels, prior_weight=prior_weight, seen=seen, only=only)

    def query_playlist_topn_capped(self, local_rows, topn: int, max_per_group: int, lam=1.0, pool=None, exclude=None, where=None,
                                   weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None,
                                   seen=None, only=None):
        return self._playlist(_np_rows(local_rows), topn, exclude, where, weights, "_capped", lam=lam, pool=pool,
                              max_per_group=max_per_group, return_mmr=return_mmr, return_pool_rows=return_pool_rows,
                              labels=labels, prior_weight=prior_weight, seen=seen, only=only)

    def fetch_rows(self, local_rows) -> np.ndarray:
        """The features of the listed rows (any order, duplicates allowed), gathered on the device: (len, 12) float32."""
        rows = _np_rows(local_rows)
        out = np.empty((rows.size, capi.DIM), dtype=np.float32)
        capi.check(self._lib.mi355rec_fetch_rows(self._h, rows.ctypes.data_as(ctypes.c_void_p), int(rows.size),
                                                 out.ctypes.data_as(ctypes.c_void_p)), self._h)
        return out

    def playlist_counters(self) -> dict:
        q, r = ctypes.c_int64(0), ctypes.c_int64(0)
        capi.check(self._lib.mi355rec_playlist_counters(self._h, ctypes.byref(q), ctypes.byref(r)), self._h)
        return {"queries": q.value, "rows_exact": r.value}


class NodeEngine(_RequestFamily):
    """The catalogue on the GPUs of one node driven by ONE process (mi355rec_create_placed): what the C++
    Recommender shim uses.  `placement`: capi.PLACEMENT_SHARDED (rows split over the devices; the default),
    PLACEMENT_REPLICATED (every device holds all rows and serves whole windows of the stream).
    `devices=None` -> devices 0 .. n_devices-1, n_devices = 0 letting the library choose; a list may repeat a
    device (virtual shards / replicas on a one-GPU box)."""

    _prefix = "mi355rec_sharded_"

    def __init__(self, feats, devices=None, n_devices: int = 0, placement: int = capi.PLACEMENT_SHARDED):
        self._lib = capi.lib()
        self._h = ctypes.c_void_p()
        arr = _np_f32(feats)
        if arr.ndim != 2 or arr.shape[1] != capi.DIM:
            raise ValueError("catalogue must be float32 [n, 12]")
        devs = None if devices is None else np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
        rc = self._lib.mi355rec_create_placed(
            arr.ctypes.data_as(ctypes.c_void_p), arr.shape[0], arr.shape[1],
            devs.ctypes.data_as(ctypes.c_void_p) if devs is not None else None,
            len(devs) if devs is not None else int(n_devices), int(placement), ctypes.byref(self._h))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._lib.mi355rec_sharded_last_error(None) or b"").decode("utf-8", "replace"))
        self.rows = int(arr.shape[0])

    def placement(self) -> int:
        return int(self._lib.mi355rec_sharded_placement(self._h))

    def _check(self, rc: int) -> None:
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._lib.mi355rec_sharded_last_error(self._h) or b"").decode("utf-8", "replace"))

    def row_set(self, ids) -> RowSet:
        """A ROW SET of this node handle from global ids (0 <= id < rows), usable on it as `seen=` or `only=`."""
        return RowSet(self, ids, self._lib.mi355rec_sharded_rowset_create)

    def _set_check(self, rc: int) -> None:
        self._check(rc)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._close_sets()
            self._lib.mi355rec_sharded_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self) -> dict:
        n, t = ctypes.c_int(0), ctypes.c_int(0)
        rows = ctypes.c_int64(0)
        devs = np.zeros(64, dtype=np.int32)
        per = np.zeros(64, dtype=np.int64)
        self._check(self._lib.mi355rec_sharded_info(self._h, ctypes.byref(n), ctypes.byref(t), ctypes.byref(rows),
                                                    devs.ctypes.data_as(ctypes.c_void_p), per.ctypes.data_as(ctypes.c_void_p)))
        return {"n_shards": n.value, "transport": t.value, "rows": rows.value,
                "devices": devs[: n.value].tolist(), "shard_rows": per[: n.value].tolist()}

    def set_transport(self, transport: int) -> None:
        self._check(self._lib.mi355rec_sharded_set_transport(self._h, int(transport)))

    def query_row_topn(self, global_row: int, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        n_out = max(int(topn), 1)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        self._check(self._lib.mi355rec_sharded_query_row_topn(
            self._h, int(global_row), int(topn), idx.ctypes.data_as(ctypes.c_void_p),
            score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)))
        return idx[:count.value].copy(), score[:count.value].copy()

    def query_topn(self, query, exclude_global: int, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _np_f32(query).reshape(capi.DIM)
        n_out = max(int(topn), 1)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        self._check(self._lib.mi355rec_sharded_query_topn(
            self._h, q.ctypes.data_as(ctypes.c_void_p), int(exclude_global), int(topn),
            idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)))
        return idx[:count.value].copy(), score[:count.value].copy()

    def query_batch_topn(self, queries, exclude_global, topn: int):
        q = _np_f32(queries).reshape(-1, capi.DIM)
        b = q.shape[0]
        excl = None
        if exclude_global is not None:
            excl = np.ascontiguousarray(np.asarray(exclude_global, dtype=np.int64).reshape(b))
        n_out = max(int(topn), 1)
        idx = np.empty((b, n_out), dtype=np.int64)
        score = np.empty((b, n_out), dtype=np.float32)
        counts = np.zeros(b, dtype=np.int32)
        self._check(self._lib.mi355rec_sharded_query_batch_topn(
            self._h, q.ctypes.data_as(ctypes.c_void_p), b,
            excl.ctypes.data_as(ctypes.c_void_p) if excl is not None else None, int(topn),
            idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p),
            counts.ctypes.data_as(ctypes.c_void_p)))
        return idx, score, counts

    # ---- LABELS (include/mi355rec_diag.h): label-filtered top-N over the whole node ----
    def query_row_topn_labels(self, global_row: int, labels, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        return _labels_query(self._lib.mi355rec_sharded_query_row_topn_labels, self._h, self._check, (int(global_row),), labels, topn)

    def query_topn_labels(self, query, exclude_global: int, labels, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _np_f32(query).reshape(capi.DIM)
        return _labels_query(self._lib.mi355rec_sharded_query_topn_labels, self._h, self._check,
                             (q.ctypes.data_as(ctypes.c_void_p), int(exclude_global)), labels, topn)

    # ---- the by-row forms of the request family (_RequestFamily): the members are global rows ----
    def query_playlist_topn(self, global_rows, topn: int, exclude=None, where=None, weights=None, labels=None, prior_weight=None,
                            scales=None, seen=None, only=None) -> Tuple[np.ndarray, np.ndarray]:
        return self._playlist(_np_rows(global_rows), topn, exclude, where, weights, labels=labels, prior_weight=prior_weight, scales=scales,
                              seen=seen, only=only)

    def query_playlist_topn_capped(self, global_rows, topn: int, max_per_group: int, lam=1.0, pool=None, exclude=None, where=None,
                                   weights=None, return_mmr=False, return_pool_rows=False, labels=None, prior_weight=None,
                                   seen=None, only=None):
        return self._playlist(_np_rows(global_rows), topn, exclude, where, weights, "_capped", lam=lam, pool=pool,
                              max_per_group=max_per_group, return_mmr=return_mmr, return_pool_rows=return_pool_rows,
                              labels=labels, prior_weight=prior_weight, seen=seen, only=only)

    def query_playlist_topn_diverse(self, global_rows, topn: int, lam, pool=None, exclude=None, where=None, weights=None,
                                    return_mmr=False, labels=None, prior_weight=None, seen=None, only=None):
        return self._playlist(_np_rows(global_rows), topn, exclude, where, weights, "_diverse", lam=lam, pool=pool, return_mmr=return_mmr,
                              labels=labels, prior_weight=prior_weight, seen=seen, only=only)

    def update_rows(self, global_rows, feats) -> None:
        """Rows change in place on every shard or replica that holds them (mi355rec_sharded_update_rows); the node owns its rows, so
        feats ([len(global_rows), 12] float32) is required.  Closes the open window and drains the workers first."""
        rows = np.ascontiguousarray(np.asarray(global_rows, dtype=np.int64).reshape(-1))
        arr = None if feats is None else _np_f32(feats).reshape(-1, capi.DIM)
        if arr is not None and arr.shape[0] != rows.size:
            raise ValueError(f"{arr.shape[0]} feature rows for {rows.size} row ids")
        self._check(self._lib.mi355rec_sharded_update_rows(
            self._h, rows.ctypes.data_as(ctypes.c_void_p) if rows.size else None, rows.size,
            None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)))

    def scores_row(self, global_row: int) -> np.ndarray:
        out = np.empty(self.rows, dtype=np.float32)
        self._check(self._lib.mi355rec_sharded_scores_row(self._h, int(global_row), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- the stream of single queries (asynchronous; tickets) ---------------------------
    def set_window(self, window: int) -> None:
        self._check(self._lib.mi355rec_sharded_set_window(self._h, int(window)))

    def set_window_mode(self, batched: bool) -> None:
        self._check(self._lib.mi355rec_sharded_set_window_mode(self._h, 1 if batched else 0))

    def enqueue_row(self, global_row: int, topn: int) -> int:
        t = ctypes.c_int64(-1)
        self._check(self._lib.mi355rec_sharded_enqueue_row(self._h, int(global_row), int(topn), ctypes.byref(t)))
        return int(t.value)

    def enqueue_query(self, query, exclude_global: int, topn: int) -> int:
        q = _np_f32(query).reshape(capi.DIM)
        t = ctypes.c_int64(-1)
        self._check(self._lib.mi355rec_sharded_enqueue_query(self._h, q.ctypes.data_as(ctypes.c_void_p), int(exclude_global),
                                                            int(topn), ctypes.byref(t)))
        return int(t.value)

    def enqueue_flush(self) -> None:
        self._check(self._lib.mi355rec_sharded_enqueue_flush(self._h))

    def wait(self, ticket: int, topn: int) -> Tuple[np.ndarray, np.ndarray]:
        idx = np.empty(int(topn), dtype=np.int64)
        score = np.empty(int(topn), dtype=np.float32)
        count = ctypes.c_int(0)
        self._check(self._lib.mi355rec_sharded_wait(self._h, int(ticket), idx.ctypes.data_as(ctypes.c_void_p),
                                                   score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)))
        return idx[:count.value].copy(), score[:count.value].copy()

    def stream_stats(self) -> dict:
        q, e, ns = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.mi355rec_sharded_stream_stats(self._h, ctypes.byref(q), ctypes.byref(e), ctypes.byref(ns)))
        return {"queries": int(q.value), "exchanges": int(e.value), "host_ns": int(ns.value)}

    def set_timing(self, enabled) -> None:
        self._check(self._lib.mi355rec_sharded_set_timing(self._h, int(enabled)))

    def shard_stats(self, shard: int) -> capi.Stats:
        st = capi.Stats()
        self._check(self._lib.mi355rec_sharded_shard_stats(self._h, int(shard), ctypes.byref(st)))
        return st

    def set_replica(self, mode: int) -> None:
        self._check(self._lib.mi355rec_sharded_set_replica(self._h, int(mode)))

    def rccl_ranks(self) -> dict:
        """What RCCL reports about the RCCL transport's communicators (mi355rec_sharded_rccl_ranks): how many the handle holds,
        ncclCommCount of the first, and whether all of them agree (0 / 0 / False until that transport has been used)."""
        comms, ranks, agree = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.mi355rec_sharded_rccl_ranks(self._h, ctypes.byref(comms), ctypes.byref(ranks), ctypes.byref(agree)))
        return {"communicators": int(comms.value), "ranks": int(ranks.value), "ranks_agree": bool(agree.value)}

    def rows_by_pointer(self) -> bool:
        return bool(self._lib.mi355rec_sharded_rows_by_pointer(self._h))

    def note(self) -> str:
        return (self._lib.mi355rec_sharded_note(self._h) or b"").decode("utf-8", "replace")


# ---- pairs of streamed queries -----------------------------------------------

def set_stream_pairing(engine: "CosineEngine", mode: int) -> None:
    """capi.PAIRING_AUTO / PAIRING_OFF / PAIRING_ON / PAIRING_GROUPS for `engine` (mi355rec_set_stream_pairing): whether two
    queued streamed queries over the 8-bit replica that ask for the same topn <= 128 share ONE pass over it — and, under
    GROUPS, whether two such pairs share one launch.  The stream then runs up to three calls behind instead of one (seven
    under GROUPS for queries by row and by value); results are unchanged.  A lane inherits the mode when it is created."""
    capi.check(engine._lib.mi355rec_set_stream_pairing(engine._h, int(mode)), engine._h)


def stream_pair_launches(engine: "CosineEngine") -> int:
    """Pairs launched by `engine` since create (mi355rec_stats_t::stream_pair_launches; a group launch adds two)."""
    return int(engine.stats().stream_pair_launches)


def stream_group_launches(engine: "CosineEngine") -> int:
    """Launches of `engine` that served two pairs, since create (mi355rec_stats_t::stream_group_launches)."""
    return int(engine.stats().stream_group_launches)


# ---- packed keys on the host (pure bit manipulation, mirrors kernels.hip.h) ----

def unpack_keys(keys) -> Tuple[np.ndarray, np.ndarray]:
    """(row, score) arrays from packed uint64/int64 keys; empty keys dropped."""
    k = np.asarray(keys).astype(np.uint64, copy=False).reshape(-1)
    k = k[k != 0]
    rows = (~k.astype(np.uint32)).astype(np.int64)  # low 32 bits = ~row
    hi = (k >> np.uint64(32)).astype(np.uint32)
    neg = (hi & np.uint32(0x80000000)) == 0
    bits = np.where(neg, ~hi, hi & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    return rows, bits.view(np.float32)


# ---- row sharding -----------------------------------------------------------

def shard_bounds(n_rows: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous row block of `rank`: [lo, hi).

    Balanced: the first n_rows % world_size ranks hold one row more, so a rank is
    empty only when n_rows < world_size (a ceil-division split leaves trailing
    ranks empty much earlier, e.g. 10 rows over 8 ranks).  An empty rank takes
    part in the collective with an all-zero key list (`ShardedEngine(local=None)`).
    """
    n, w, r = int(n_rows), int(world_size), int(rank)
    per, rem = divmod(n, w)
    lo = r * per + min(r, rem)
    hi = lo + per + (1 if r < rem else 0)
    return lo, hi


class ShardedEngine:
    """Row-sharded catalogue, one process per GPU, one all-gather per query.

    `local` is this rank's engine over rows [lo, hi) created with
    row_base=lo, so the keys it emits already carry GLOBAL row ids and the
    merged result does not depend on the number of ranks.  Everything is
    enqueued on the current stream; nothing synchronises the host.
    """

    def __init__(self, local, max_topn: int, group=None, device=None, always_gather: bool = False, lanes: int = 1):
        """lanes > 1: the windowed stream of single queries is dealt over that many lanes of `local` (CosineEngine.lane(): the
        same rows and replicas, own stream state), each on its own stream — a rank's launches then overlap as on one GPU."""
        import torch
        import torch.distributed as dist

        self._torch = torch
        self._dist = dist
        self.local = local
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.max_topn = int(max_topn)
        if not 1 <= self.max_topn <= capi.MAX_TOPN_FAST:
            # the merge of the gathered lists is a single launch (mi355rec_enqueue_merge_keys)
            raise ValueError(f"max_topn must be in [1, {capi.MAX_TOPN_FAST}], got {max_topn}")
        self.always_gather = bool(always_gather)  # run the collective even at world size 1
        # RCCL gathers device tensors directly.  Under gloo (CPU rehearsals, or several
        # ranks sharing one GPU in a test) the keys are staged through host memory.
        self._stage_host = str(dist.get_backend(group)).lower() == "gloo" and torch.device(
            device if device is not None else "cuda").type == "cuda"
        dev = device if device is not None else torch.device("cuda", local.device)
        self.device = dev
        self._lanes = [local]
        self._lane_streams = [None]
        # The windowed stream gathers a window a fixed number of calls into the next one: it counts on the rank's streamed
        # queries running ONE call behind, so the rank's engine does not pair them (its lanes inherit that).
        if isinstance(local, CosineEngine):
            set_stream_pairing(local, capi.PAIRING_OFF)
        if int(lanes) > 1 and hasattr(local, "lane"):
            self._lanes = [local] + [local.lane() for _ in range(int(lanes) - 1)]
            self._lane_streams = [ln.own_stream() for ln in self._lanes]
            self._lane_ev = [torch.cuda.Event() for _ in self._lanes]      # "this lane's launches so far" -> the collective's stream
            self._buf_ev = [None, None]                                    # "window buffer b has been gathered" -> the lanes
        self._w_calls = 0
        self.local_keys = torch.zeros(self.max_topn, dtype=torch.int64, device=dev)
        self.gathered = torch.zeros(self.world * self.max_topn, dtype=torch.int64, device=dev)
        self.out_keys = torch.zeros(self.max_topn, dtype=torch.int64, device=dev)
        self.out_idx = torch.full((self.max_topn,), -1, dtype=torch.int64, device=dev)
        self.out_score = torch.zeros(self.max_topn, dtype=torch.float32, device=dev)

    def _all_gather(self, gathered, local) -> None:
        if not self._stage_host:
            self._dist.all_gather_into_tensor(gathered, local, group=self.group)
            return
        host_out = self._torch.empty(gathered.shape, dtype=gathered.dtype)
        self._dist.all_gather_into_tensor(host_out, local.cpu(), group=self.group)
        gathered.copy_(host_out)

    def enqueue_query(self, query, exclude_global: int, topn: int) -> None:
        """Scan the local shard, all-gather the candidates, merge on device."""
        if topn > self.max_topn:
            raise ValueError(f"topn {topn} > max_topn {self.max_topn}")
        k = int(topn)
        local = self.local_keys[:k]
        self.local.enqueue_query_keys(query, exclude_global, k, local)
        if self.world == 1 and not self.always_gather:
            gathered = local
        else:
            gathered = self.gathered[: self.world * k]
            self._all_gather(gathered, local)
        self.local.enqueue_merge_keys(gathered, self.world, k, k, self.out_keys[:k],
                                      self.out_idx[:k], self.out_score[:k])

    # -- windowed single queries: one all-gather per `window` queries ---------------
    def enqueue_query_windowed(self, query, exclude_global: int, topn: int, window: int = 16) -> int:
        """A stream of single queries on a sharded catalogue: every query is still one
        full pass over every shard, but the exchange is amortised — the local merge of
        query k rides in the scan launch of query k + 1 (streamed C-ABI calls) and the
        per-rank key lists of `window` queries cross xGMI in ONE all-gather followed by ONE
        batched merge launch.

        The local stream is NOT drained when a window fills: a streamed query's keys are complete, in stream
        order, behind the second streamed call after it (the stream runs one call behind and its merge rides in
        the launch after that; csrc/sharded.hip keeps the same lag, kWindowLag), so a full window's all-gather
        is enqueued two queries into the NEXT window.  Returns the number of queries whose results became
        available during this call (0 or `window`): they are in `self.window_keys / window_idx / window_score`
        ([count, topn]; also appended to `self.merged_windows`, which every call resets).  `flush_window`
        closes what is left."""
        torch = self._torch
        k, w = int(topn), int(window)
        if k > self.max_topn:
            raise ValueError(f"topn {topn} > max_topn {self.max_topn}")
        self.merged_windows = []
        if getattr(self, "_w_shape", None) != (w, k):
            if getattr(self, "_w_count", 0) or getattr(self, "_w_pending", None) is not None:
                self.flush_window()
                self.merged_windows = []
            dev = self.device
            self._w_local = [torch.zeros(w * k, dtype=torch.int64, device=dev) for _ in range(2)]
            self._w_gather = [torch.zeros(self.world * w * k, dtype=torch.int64, device=dev) for _ in range(2)]
            self._w_keys = [torch.zeros(w * k, dtype=torch.int64, device=dev) for _ in range(2)]
            self._w_idx = [torch.full((w * k,), -1, dtype=torch.int64, device=dev) for _ in range(2)]
            self._w_score = [torch.zeros(w * k, dtype=torch.float32, device=dev) for _ in range(2)]
            self._w_shape = (w, k)
            if len(self._lanes) > 1:   # (the lanes' streams do not wait for the stream that just zeroed these buffers)
                torch.cuda.current_stream().synchronize()
                self._buf_ev = [None, None]
            # a real engine underneath (not a test double): the call bound once — output pointers per slot instead of a tensor
            # slice per query, the handle and the lane's stream resolved here (this loop is what every rank runs per query:
            # 15 us of Python per query made eight ranks no faster than one)
            self._w_fast = None
            if all(hasattr(ln, "_h") and hasattr(ln, "_lib") for ln in self._lanes):
                self._w_ptrs = [[ctypes.c_void_p(t.data_ptr() + s * k * 8) for s in range(w)] for t in self._w_local]
                self._w_fast = [(ln._lib.mi355rec_enqueue_query_keys_streamed, ln._h,
                                 ln._stream_ptr(ls) if ls is not None else None) for ln, ls in zip(self._lanes, self._lane_streams)]
            self._w_count = 0
            self._w_cur = 0
            self._w_pending = None
        slot, buf = self._w_count, self._w_cur
        nl = len(self._lanes)
        lane = self._w_calls % nl
        self._w_calls += 1
        if nl > 1 and slot == 0 and self._buf_ev[buf] is not None:
            for ls in self._lane_streams:   # this buffer's previous window has been gathered before a lane writes to it again
                ls.wait_event(self._buf_ev[buf])
        if self._w_fast is not None:
            fn, h, sp = self._w_fast[lane]
            q = query if (isinstance(query, np.ndarray) and query.dtype == np.float32 and query.size == capi.DIM
                          and query.flags.c_contiguous) else _np_f32(query).reshape(capi.DIM)
            rc = fn(h, ctypes.c_void_p(q.ctypes.data), int(exclude_global), k, self._w_ptrs[buf][slot],
                    sp if sp is not None else CosineEngine._stream_ptr(None))
            if rc:
                capi.check(rc, h)
        elif nl > 1:
            self._lanes[lane].enqueue_query_keys_streamed(query, exclude_global, k, self._w_local[buf][slot * k:(slot + 1) * k],
                                                          stream=self._lane_streams[lane])
        else:
            self.local.enqueue_query_keys_streamed(query, exclude_global, k, self._w_local[buf][slot * k:(slot + 1) * k])
        self._w_count += 1
        done = 0
        lag = 2 * nl   # a lane runs one call behind and its merge rides in the call after that: two calls PER LANE
        if self._w_pending is not None and self._w_count >= lag:   # the window before is complete behind this call
            done = self._merge_window(*self._w_pending)
            self._w_pending = None
        if self._w_count == w:
            if w >= lag + 1:   # (a smaller window would fill again before its predecessor is `lag` calls old)
                self._w_pending = (buf, w)
                self._w_cur = 1 - buf
                self._w_count = 0
            else:
                done = self.flush_window()
        return done

    def _merge_window(self, buf: int, cnt: int) -> int:
        """ONE all-gather + ONE batched merge for the `cnt` queries of window buffer `buf` (its local key lists are
        complete in stream order)."""
        w, k = self._w_shape
        need = cnt * k
        local = self._w_local[buf][:need]
        if len(self._lanes) > 1:   # the collective's stream waits for what every lane has been given so far
            cur = self._torch.cuda.current_stream()
            for ls, ev in zip(self._lane_streams, self._lane_ev):
                ev.record(ls)
                cur.wait_event(ev)
        if self.world == 1 and not self.always_gather:
            gathered = local
        else:
            gathered = self._w_gather[buf][: self.world * need]
            self._all_gather(gathered, local)
        self.local.enqueue_merge_keys_batch(gathered, self.world, k, need, k, cnt, k, self._w_keys[buf][:need],
                                            self._w_idx[buf][:need], self._w_score[buf][:need])
        if len(self._lanes) > 1:
            ev = self._torch.cuda.Event()
            ev.record(self._torch.cuda.current_stream())
            self._buf_ev[buf] = ev
        self.window_keys = self._w_keys[buf][:need].view(cnt, k)
        self.window_idx = self._w_idx[buf][:need].view(cnt, k)
        self.window_score = self._w_score[buf][:need].view(cnt, k)
        if not hasattr(self, "merged_windows"):
            self.merged_windows = []
        self.merged_windows.append((self.window_keys, self.window_idx, self.window_score))
        return cnt

    def flush_window(self) -> int:
        """Closes the stream of windows: drains the local pipeline, then merges the window that was still waiting
        for its lag (if any) and the open, possibly partial one — each ONE all-gather + ONE batched merge.  Returns
        the number of queries of the LAST window merged (0: nothing was outstanding); `self.merged_windows` lists
        the results of every window this call merged, oldest first."""
        self.merged_windows = []
        cnt = getattr(self, "_w_count", 0)
        pending = getattr(self, "_w_pending", None)
        if cnt == 0 and pending is None:
            return 0
        for ln, ls in zip(self._lanes, self._lane_streams):
            ln.enqueue_flush(stream=ls) if ls is not None else ln.enqueue_flush()
        done = 0
        if pending is not None:
            done = self._merge_window(*pending)
            self._w_pending = None
        if cnt:
            done = self._merge_window(self._w_cur, cnt)
            self._w_count = 0
        return done

    def enqueue_batch(self, queries, exclude_global, topn: int):
        """`batch` queries: local multi-query passes, ONE all-gather of batch*topn
        keys per rank, one merge launch (a workgroup per query).  Results in
        self.batch_keys / batch_idx / batch_score ([batch, topn])."""
        torch = self._torch
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32).reshape(-1, 12))
        b, k = q.shape[0], int(topn)
        need = b * k
        if getattr(self, "_batch_cap", 0) < need:
            dev = self.device
            self._b_local = torch.zeros(need, dtype=torch.int64, device=dev)
            self._b_gather = torch.zeros(self.world * need, dtype=torch.int64, device=dev)
            self._b_keys = torch.zeros(need, dtype=torch.int64, device=dev)
            self._b_idx = torch.full((need,), -1, dtype=torch.int64, device=dev)
            self._b_score = torch.zeros(need, dtype=torch.float32, device=dev)
            self._batch_cap = need
        local = self._b_local[:need]
        self.local.enqueue_batch_keys(q, exclude_global, k, local)
        if self.world == 1 and not self.always_gather:
            gathered = local
        else:
            gathered = self._b_gather[: self.world * need]
            self._all_gather(gathered, local)
        self.local.enqueue_merge_keys_batch(gathered, self.world, k, need, k, b, k, self._b_keys[:need],
                                            self._b_idx[:need], self._b_score[:need])
        self.batch_keys = self._b_keys[:need].view(b, k)
        self.batch_idx = self._b_idx[:need].view(b, k)
        self.batch_score = self._b_score[:need].view(b, k)

    def query(self, query, exclude_global: int, topn: int):
        """Synchronous convenience wrapper: (rows, scores) as numpy arrays."""
        self.enqueue_query(query, exclude_global, topn)
        idx = self.out_idx[:topn].cpu().numpy()
        score = self.out_score[:topn].cpu().numpy()
        keep = idx >= 0
        return idx[keep], score[keep]
