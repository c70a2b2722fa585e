"""ctypes binding of the C-ABI in include/mi355rec.h (core) and include/mi355rec_diag.h (statistics, controls, hooks).

This is plumbing only: every compute call goes to the HIP library.  If the
library is missing the import of :func:`lib` raises — there is no Python or CPU
fallback for the hot path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from pathlib import Path

PKG = Path(__file__).resolve().parent
# MI355REC_LIB: another build of the same C-ABI (tests/test_gpu_experiments.py runs the A/B routes of the MI355REC_EXPERIMENTS
# build this way, in a child process; the product never sets it)
LIB_PATH = Path(os.environ["MI355REC_LIB"]) if os.environ.get("MI355REC_LIB") else PKG / "libmi355rec.so"

DIM = 12
MAX_TOPN_FAST = 1024
BATCH_AUTO, BATCH_MULTI, BATCH_MFMA, BATCH_HALF, BATCH_Q8, BATCH_MFMA_NOSKIP = 0, 1, 2, 3, 4, 5
REPLICA_AUTO, REPLICA_OFF, REPLICA_ON, REPLICA_FP16 = 0, 1, 2, 3
SAMPLE_AUTO, SAMPLE_STRIDED, SAMPLE_BUCKETED = 0, 1, 2   # mi355rec_set_sample
SAMPLE_AUTO_MIN_ROWS = 6_000_000
PAIRING_AUTO, PAIRING_OFF, PAIRING_ON, PAIRING_GROUPS = 0, 1, 2, 3   # mi355rec_set_stream_pairing
PAIRING_AUTO_MIN_ROWS = 2_500_000
GROUPS_AUTO_MIN_ROWS = 2_500_000
TRANSPORT_PEER, TRANSPORT_RCCL = 1, 2
PLACEMENT_AUTO, PLACEMENT_SHARDED, PLACEMENT_REPLICATED, PLACEMENT_CPU = 0, 1, 2, 3
CREATE_NO_REPLICA = 1
DEBUG_HANDOFF_POISON, DEBUG_HANDOFF_DROP_STORES, DEBUG_HANDOFF_NO_LAST_RIDER = 1, 2, 4
BUILD_EXPERIMENTS, BUILD_PHASE_CLOCK, BUILD_TEST_HOOKS = 1, 2, 4
PROBE_FP32_ROWS, PROBE_FP16_REPLICA, PROBE_Q8_REPLICA = 0, 1, 2

OK = 0
ERR_INVALID_ARG = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_OUT_OF_MEMORY = -4
MAX_LABELS = 1024
MAX_PLAYLIST = 32
MAX_EXCLUDE = 1024
# FEATURE FILTERS: the catalogue's columns in matrix order (Song.h); `where=` mappings take a name or an index.
FEATURE_NAMES = ("danceability", "energy", "key", "loudness", "mode", "speechiness", "acousticness", "instrumentalness",
                 "liveness", "valence", "tempo", "genre_id")


class Filter(ctypes.Structure):
    """mi355rec_filter_t (include/mi355rec_diag.h, FEATURE FILTERS)."""
    _fields_ = [("active", c_uint32), ("lo", c_float * DIM), ("hi", c_float * DIM)]


PQ_DIVERSE, PQ_CAPPED, PQ_PRIOR = 1, 2, 4
MAX_PRIOR_WEIGHT = 4.0
MAX_FEATURE_SCALE = 1024.0   # MI355REC_MAX_FEATURE_SCALE (FEATURE SCALES)


class PlaylistQuery(ctypes.Structure):
    """mi355rec_playlist_query_t (include/mi355rec_diag.h, PLAYLIST REQUESTS); `size` is sizeof of this struct."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("members", c_void_p), ("rows", c_void_p), ("weights", c_void_p),
                ("exclude_global", c_void_p), ("filter", POINTER(Filter)), ("labels", c_void_p), ("k", c_int32),
                ("n_exclude", c_int32), ("n_labels", c_int32), ("topn", c_int32), ("lambda_", c_float), ("pool", c_int32),
                ("max_per_group", c_int32), ("prior_weight", c_float)]


class PlaylistResult(ctypes.Structure):
    """mi355rec_playlist_result_t: every pointer but out_idx may be NULL."""
    _fields_ = [("out_idx", c_void_p), ("out_score", c_void_p), ("out_mmr", c_void_p), ("out_count", POINTER(c_int)),
                ("out_pool_rows", POINTER(c_int))]


# The four metric requests (distance, any-of, Manhattan, Jaccard) are one 64-byte layout under four names in the C-ABI: four classes here.
_METRIC_QUERY_FIELDS = [("size", c_uint32), ("flags", c_uint32), ("members", c_void_p), ("rows", c_void_p), ("exclude_global", c_void_p),
                        ("filter", POINTER(Filter)), ("labels", c_void_p), ("k", c_int32), ("n_exclude", c_int32), ("n_labels", c_int32),
                        ("topn", c_int32)]


class DistanceQuery(ctypes.Structure):
    """mi355rec_distance_query_t (include/mi355rec_diag.h, DISTANCE REQUESTS); `size` is sizeof of this struct, flags 0."""
    _fields_ = _METRIC_QUERY_FIELDS


class DistanceResult(ctypes.Structure):
    """mi355rec_distance_result_t: every pointer but out_idx may be NULL."""
    _fields_ = [("out_idx", c_void_p), ("out_distance", c_void_p), ("out_count", POINTER(c_int))]


class AnyOfQuery(ctypes.Structure):
    """mi355rec_anyof_query_t (include/mi355rec_diag.h, ANY-OF REQUESTS); `size` is sizeof of this struct, flags 0."""
    _fields_ = _METRIC_QUERY_FIELDS


class AnyOfResult(ctypes.Structure):
    """mi355rec_anyof_result_t: every pointer but out_idx may be NULL; out_member holds int32."""
    _fields_ = [("out_idx", c_void_p), ("out_score", c_void_p), ("out_member", c_void_p), ("out_count", POINTER(c_int))]


class ManhattanQuery(ctypes.Structure):
    """mi355rec_manhattan_query_t (include/mi355rec_diag.h, MANHATTAN REQUESTS); `size` is sizeof of this struct, flags 0."""
    _fields_ = _METRIC_QUERY_FIELDS


class ManhattanResult(ctypes.Structure):
    """mi355rec_manhattan_result_t: every pointer but out_idx may be NULL; out_distance holds m(x)."""
    _fields_ = [("out_idx", c_void_p), ("out_distance", c_void_p), ("out_count", POINTER(c_int))]


class JaccardQuery(ctypes.Structure):
    """mi355rec_jaccard_query_t (include/mi355rec_diag.h, JACCARD REQUESTS); `size` is sizeof of this struct, flags 0."""
    _fields_ = _METRIC_QUERY_FIELDS


class JaccardResult(ctypes.Structure):
    """mi355rec_jaccard_result_t: every pointer but out_idx may be NULL; out_similarity holds v(x)."""
    _fields_ = [("out_idx", c_void_p), ("out_similarity", c_void_p), ("out_count", POINTER(c_int))]


BOUNDED_COSINE, BOUNDED_EUCLIDEAN = 0, 1  # mi355rec_bounded_query_t::metric


class BoundedQuery(ctypes.Structure):
    """mi355rec_bounded_query_t (include/mi355rec_diag.h, BOUNDED REQUESTS): the metric requests' 64 bytes, then `metric` and `bound`
    (72 bytes); `size` is sizeof of this struct, flags 0, topn 0 counts only."""
    _fields_ = _METRIC_QUERY_FIELDS + [("metric", c_int32), ("bound", c_float)]


class BoundedResult(ctypes.Structure):
    """mi355rec_bounded_result_t: out_total (int64) is required; out_idx and out_score may be NULL when topn == 0; out_count may be NULL."""
    _fields_ = [("out_idx", c_void_p), ("out_score", c_void_p), ("out_count", POINTER(c_int)), ("out_total", POINTER(c_int64))]


ROWSET_EXCLUDE, ROWSET_ONLY = 0, 1   # MI355REC_ROWSET_* (ROW SETS)
MAX_CANDIDATES = 1 << 20             # MI355REC_MAX_CANDIDATES (CANDIDATE LISTS)


class RequestExt(ctypes.Structure):
    """mi355rec_request_ext_t (include/mi355rec_diag.h, ROW SETS): the per-request extras beside the two request structs; `size` is
    sizeof of this struct (24).  feature_scales: NULL or 12 floats; rowset: NULL or a mi355rec_rowset_t*."""
    _fields_ = [("size", c_uint32), ("rowset_mode", c_uint32), ("feature_scales", c_void_p), ("rowset", c_void_p)]


class BucketSampleInfo(ctypes.Structure):   # mi355rec_bucket_sample_info_t
    _fields_ = [("base_rows", c_int64), ("regions", c_int32), ("centroids", c_int32), ("bytes", c_int64), ("stride_rows", c_int64),
                ("centroid_stride", c_int64), ("picks", c_int32), ("mode", c_int32), ("last_used", c_int32), ("build_ms", c_float)]


class UpdateInfo(ctypes.Structure):   # mi355rec_update_info_t (size = sizeof of this struct, 32, on entry)
    _fields_ = [("size", c_uint32), ("last_ms", c_float), ("calls", c_int64), ("rows", c_int64), ("rows_since_snapshot", c_int64)]


class Stats(ctypes.Structure):
    _fields_ = [
        ("rows", c_int64),
        ("row_base", c_int64),
        ("device", c_int32),
        ("compute_units", c_int32),
        ("grid_blocks", c_int32),
        ("block_threads", c_int32),
        ("bytes_per_query", c_int64),
        ("last_scan_ms", c_float),
        ("last_merge_ms", c_float),
        ("last_pass_ms", c_float),
        ("batched_grid_blocks", c_int32),
        ("batched_margin", c_float),
        ("replica_bytes_per_query", c_int64),
        ("replica_active", c_int32),
        ("replica_grid_blocks", c_int32),
        ("replica_build_ms", c_float),
        ("replica_margin_single", c_float),
        ("replica_margin_multi", c_float),
        ("replica_single_bytes_per_query", c_int64),
        ("replica_single_row_bytes", c_int32),
        ("lone_fused_queries", c_int32),
        ("route_fp32", c_int64),
        ("route_fp16", c_int64),
        ("route_q8", c_int64),
        ("route_q8_lone", c_int64),
        ("route_multi_fp32", c_int64),
        ("route_multi_fp16", c_int64),
        ("route_multi_q8", c_int64),
        ("route_mfma_two_pass", c_int64),
        ("route_exact_queue", c_int64),
        ("device_bytes_per_row", c_int32),
        ("stream_pair_launches", c_int64),
        ("stream_group_launches", c_int64),
    ]


# name -> (restype, argtypes); mirrors include/mi355rec.h one to one
SIGNATURES = {
    "mi355rec_build_flags": (c_int, []),
    "mi355rec_device_count": (c_int, []),
    "mi355rec_last_global_error": (c_char_p, []),
    "mi355rec_create": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, POINTER(c_void_p)]),
    "mi355rec_create_device": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, POINTER(c_void_p)]),
    "mi355rec_create_ex": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int, POINTER(c_void_p)]),
    "mi355rec_create_device_ex": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int, POINTER(c_void_p)]),
    "mi355rec_destroy": (None, [c_void_p]),
    "mi355rec_last_error": (c_char_p, [c_void_p]),
    "mi355rec_create_lane": (c_int, [c_void_p, POINTER(c_void_p)]),
    "mi355rec_own_stream": (c_void_p, [c_void_p]),
    "mi355rec_lane_status": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mi355rec_stats": (c_int, [c_void_p, POINTER(Stats)]),
    "mi355rec_stats_sized": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, POINTER(ctypes.c_size_t)]),
    "mi355rec_scores_row": (c_int, [c_void_p, c_int64, c_void_p]),
    "mi355rec_scores": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi355rec_query_row_topn": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_query_topn": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_query_batch_topn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mi355rec_enqueue_row_keys": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_query_keys": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_row_keys_streamed": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_query_keys_streamed": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_flush": (c_int, [c_void_p, c_void_p]),
    "mi355rec_enqueue_batch_keys": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_batch_keys_streamed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mi355rec_batch_pointers_ok": (c_int, [c_void_p, c_int]),
    "mi355rec_enqueue_batch_mixed_keys": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_batch_mixed_keys_streamed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mi355rec_enqueue_batch_keys_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mi355rec_set_batch_path": (c_int, [c_void_p, c_int]),
    "mi355rec_set_replica": (c_int, [c_void_p, c_int]),
    "mi355rec_rebuild_replica": (c_int, [c_void_p]),
    "mi355rec_replica_counters": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "mi355rec_set_sample": (c_int, [c_void_p, c_int]),
    "mi355rec_set_stream_pairing": (c_int, [c_void_p, c_int]),
    "mi355rec_bucket_sample_info": (c_int, [c_void_p, c_void_p]),
    "mi355rec_bucket_sample_rows": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi355rec_batched_last_counters": (c_int, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64),
                                               POINTER(c_int32)]),
    "mi355rec_batched_pass2_pairs": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "mi355rec_enqueue_merge_keys": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mi355rec_enqueue_merge_keys_batch": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int64, c_int, c_int,
                                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "mi355rec_enqueue_scores": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mi355rec_enqueue_stream_probe": (c_int, [c_void_p, c_void_p, c_void_p]),
    "mi355rec_enqueue_stream_probe_of": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "mi355rec_set_timing": (c_int, [c_void_p, c_int]),
    "mi355rec_fetch_row": (c_int, [c_void_p, c_int64, c_void_p]),
    "mi355rec_create_sharded": (c_int, [c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_create_sharded_on": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, POINTER(c_void_p)]),
    "mi355rec_create_placed": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_auto_shards": (c_int, [c_int64, c_int]),
    "mi355rec_sharded_placement": (c_int, [c_void_p]),
    "mi355rec_sharded_destroy": (None, [c_void_p]),
    "mi355rec_sharded_last_error": (c_char_p, [c_void_p]),
    "mi355rec_sharded_set_transport": (c_int, [c_void_p, c_int]),
    "mi355rec_sharded_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int64), c_void_p, c_void_p]),
    "mi355rec_sharded_query_row_topn": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_topn": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_batch_topn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mi355rec_sharded_scores_row": (c_int, [c_void_p, c_int64, c_void_p]),
    "mi355rec_row_ptr": (c_int, [c_void_p, c_int64, POINTER(c_void_p)]),
    "mi355rec_enqueue_ptr_keys": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mi355rec_enqueue_ptr_keys_streamed": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "mi355rec_sharded_set_timing": (c_int, [c_void_p, c_int]),
    "mi355rec_sharded_shard_stats": (c_int, [c_void_p, c_int, POINTER(Stats)]),
    "mi355rec_sharded_set_replica": (c_int, [c_void_p, c_int]),
    "mi355rec_sharded_rows_by_pointer": (c_int, [c_void_p]),
    "mi355rec_sharded_note": (c_char_p, [c_void_p]),
    "mi355rec_sharded_set_window": (c_int, [c_void_p, c_int]),
    "mi355rec_sharded_set_window_mode": (c_int, [c_void_p, c_int]),
    "mi355rec_sharded_enqueue_row": (c_int, [c_void_p, c_int64, c_int, POINTER(c_int64)]),
    "mi355rec_sharded_enqueue_query": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_int64)]),
    "mi355rec_sharded_enqueue_flush": (c_int, [c_void_p]),
    "mi355rec_sharded_wait": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_stream_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "mi355rec_debug_handoff": (c_int, [c_void_p, c_int]),
    "mi355rec_sharded_rccl_ranks": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "mi355rec_set_labels": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_query_row_topn_labels": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_query_topn_labels": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_label_counters": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "mi355rec_sharded_set_labels": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_sharded_query_row_topn_labels": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                       POINTER(c_int)]),
    "mi355rec_sharded_query_topn_labels": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                   POINTER(c_int)]),
    "mi355rec_query_mean_topn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_query_playlist_topn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_playlist_counters": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "mi355rec_sharded_query_mean_topn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                 POINTER(c_int)]),
    "mi355rec_sharded_query_playlist_topn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                     POINTER(c_int)]),
    "mi355rec_query_mean_topn_where": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                               POINTER(c_int)]),
    "mi355rec_query_playlist_topn_where": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                                   POINTER(c_int)]),
    "mi355rec_sharded_query_mean_topn_where": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                       c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_playlist_topn_where": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                           c_void_p, POINTER(c_int)]),
    "mi355rec_query_mean_topn_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                  c_void_p, POINTER(c_int)]),
    "mi355rec_query_playlist_topn_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                                      c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_mean_topn_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                                          c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_playlist_topn_weighted": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                              c_int, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_query_mean_topn_diverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int, c_int,
                                                 c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_query_playlist_topn_diverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int,
                                                     c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_mean_topn_diverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int,
                                                         c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_sharded_query_playlist_topn_diverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float,
                                                             c_int, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "mi355rec_fetch_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "mi355rec_set_groups": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_sharded_set_groups": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_query_mean_topn_capped": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int, c_int, c_int,
        c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mi355rec_query_playlist_topn_capped": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int, c_int, c_int,
        c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mi355rec_sharded_query_mean_topn_capped": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int, c_int, c_int,
        c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mi355rec_sharded_query_playlist_topn_capped": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int, c_int, c_int,
        c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mi355rec_set_priors": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_sharded_set_priors": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_query_playlist_request": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(PlaylistResult)]),
    "mi355rec_sharded_query_playlist_request": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(PlaylistResult)]),
    "mi355rec_query_distance_request": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(DistanceResult)]),
    "mi355rec_sharded_query_distance_request": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(DistanceResult)]),
    # FEATURE SCALES: the two requests with 12 per-feature factors (NULL: the unscaled call)
    "mi355rec_query_playlist_request_scaled": (c_int, [c_void_p, POINTER(PlaylistQuery), c_void_p, POINTER(PlaylistResult)]),
    "mi355rec_query_distance_request_scaled": (c_int, [c_void_p, POINTER(DistanceQuery), c_void_p, POINTER(DistanceResult)]),
    "mi355rec_sharded_query_playlist_request_scaled": (c_int, [c_void_p, POINTER(PlaylistQuery), c_void_p, POINTER(PlaylistResult)]),
    "mi355rec_sharded_query_distance_request_scaled": (c_int, [c_void_p, POINTER(DistanceQuery), c_void_p, POINTER(DistanceResult)]),
    # ROW SETS: one bit per row (a listening history, a candidate set), and the requests with their per-request extras
    "mi355rec_rowset_create": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_void_p)]),
    "mi355rec_sharded_rowset_create": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_void_p)]),
    "mi355rec_rowset_add": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_rowset_count": (c_int64, [c_void_p]),
    "mi355rec_rowset_destroy": (None, [c_void_p]),
    "mi355rec_query_playlist_request_ext": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(RequestExt), POINTER(PlaylistResult)]),
    "mi355rec_query_distance_request_ext": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(RequestExt), POINTER(DistanceResult)]),
    "mi355rec_sharded_query_playlist_request_ext": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(RequestExt), POINTER(PlaylistResult)]),
    "mi355rec_sharded_query_distance_request_ext": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(RequestExt), POINTER(DistanceResult)]),
    # CANDIDATE LISTS: the _ext requests with a list of global ids (c_void_p, c_int64): only the listed rows are gathered and ranked
    "mi355rec_query_playlist_request_candidates": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                           POINTER(PlaylistResult)]),
    "mi355rec_query_distance_request_candidates": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                           POINTER(DistanceResult)]),
    "mi355rec_sharded_query_playlist_request_candidates": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                                   POINTER(PlaylistResult)]),
    "mi355rec_sharded_query_distance_request_candidates": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                                   POINTER(DistanceResult)]),
    "mi355rec_candidates_counters": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    # CANDIDATE SCORES: the same request and list; every listed row's value (float32) and admissible flag (uint8, may be NULL) in list order
    "mi355rec_score_playlist_request_candidates": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                           c_void_p, c_void_p]),
    "mi355rec_score_distance_request_candidates": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                           c_void_p, c_void_p]),
    "mi355rec_sharded_score_playlist_request_candidates": (c_int, [c_void_p, POINTER(PlaylistQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                                   c_void_p, c_void_p]),
    "mi355rec_sharded_score_distance_request_candidates": (c_int, [c_void_p, POINTER(DistanceQuery), POINTER(RequestExt), c_void_p, c_int64,
                                                                   c_void_p, c_void_p]),
    # ANY-OF REQUESTS: top-N by the best-matching member, with the matched member's index; one entry point takes the ext
    "mi355rec_query_anyof_request": (c_int, [c_void_p, POINTER(AnyOfQuery), POINTER(RequestExt), POINTER(AnyOfResult)]),
    "mi355rec_sharded_query_anyof_request": (c_int, [c_void_p, POINTER(AnyOfQuery), POINTER(RequestExt), POINTER(AnyOfResult)]),
    # MANHATTAN REQUESTS: nearest-by-L1 top-N; one entry point takes the ext
    "mi355rec_query_manhattan_request": (c_int, [c_void_p, POINTER(ManhattanQuery), POINTER(RequestExt), POINTER(ManhattanResult)]),
    "mi355rec_sharded_query_manhattan_request": (c_int, [c_void_p, POINTER(ManhattanQuery), POINTER(RequestExt), POINTER(ManhattanResult)]),
    # BOUNDED REQUESTS: the rows at or above a score floor (within a radius) and their exact number; one entry point takes the ext
    "mi355rec_query_bounded_request": (c_int, [c_void_p, POINTER(BoundedQuery), POINTER(RequestExt), POINTER(BoundedResult)]),
    "mi355rec_sharded_query_bounded_request": (c_int, [c_void_p, POINTER(BoundedQuery), POINTER(RequestExt), POINTER(BoundedResult)]),
    # JACCARD REQUESTS: top-N by weighted (Ruzicka) Jaccard similarity; one entry point takes the ext
    "mi355rec_query_jaccard_request": (c_int, [c_void_p, POINTER(JaccardQuery), POINTER(RequestExt), POINTER(JaccardResult)]),
    "mi355rec_sharded_query_jaccard_request": (c_int, [c_void_p, POINTER(JaccardQuery), POINTER(RequestExt), POINTER(JaccardResult)]),
    # ROW UPDATES: rows change in place, every route answers as a freshly created handle would
    "mi355rec_update_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "mi355rec_sharded_update_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "mi355rec_update_info": (c_int, [c_void_p, POINTER(UpdateInfo)]),
    "mi355rec_replica_entries": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    # what a node handle is made of (host-only accessors for the companion library libmi355rec_embed.so)
    "mi355rec_sharded_shard_handle": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "mi355rec_sharded_host_rows": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "mi355rec_pack_key": (c_uint64, [c_float, c_int64]),
    "mi355rec_key_score": (c_float, [c_uint64]),
    "mi355rec_key_row": (c_int64, [c_uint64]),
}

# declared under #ifdef MI355REC_TEST_HOOKS in include/mi355rec_diag.h: absent from the product library
TEST_HOOKS = frozenset({"mi355rec_debug_handoff"})

_lib = None


def lib() -> ctypes.CDLL:
    """Load libmi355rec.so (built by ``spotify_recommender_amd.build``)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build` "
                "(hipcc --offload-arch=gfx950). The cosine top-N path has no fallback."
            )
        # One HIP runtime per process: torch bundles its own libamdhip64 and
        # whichever runtime touches the GPU first owns it.  Importing torch
        # first maps its runtime, and our library's libamdhip64.so dependency
        # then resolves to that same copy (same SONAME).  Without torch the
        # library uses /opt/rocm's runtime (the C++ CLI path).
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover
            pass
        handle = ctypes.CDLL(str(LIB_PATH))
        lenient = os.environ.get("MI355REC_CAPI_LENIENT") == "1"   # tools only: A/B against a library of an EARLIER round (--lib)
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            except AttributeError:
                if lenient or name in TEST_HOOKS:   # (test hooks: only in -DMI355REC_TEST_HOOKS builds, see has_test_hooks)
                    continue
                raise
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def has_test_hooks() -> bool:
    """True when the loaded library was built with -DMI355REC_TEST_HOOKS (libmi355rec_testhooks.so, the experiments build):
    mi355rec_debug_handoff exists.  The product library returns False."""
    L = lib()
    return hasattr(L, "mi355rec_build_flags") and bool(L.mi355rec_build_flags() & BUILD_TEST_HOOKS)


def has_experiments() -> bool:
    """True when the loaded library is an MI355REC_EXPERIMENTS build (tools/: A/B routes and environment knobs)."""
    L = lib()
    if not hasattr(L, "mi355rec_build_flags"):   # (a library of an earlier round, loaded leniently by a tool)
        return False
    return bool(L.mi355rec_build_flags() & BUILD_EXPERIMENTS)


# ---- EMBEDDING TABLES: the companion library libmi355rec_embed.so (include/mi355rec_embed.h), a second table ----
EMBED_LIB_PATH = PKG / "libmi355rec_embed.so"
EMBED_COSINE, EMBED_DOT = 0, 1
EMBED_DIMS = (16, 32, 64, 128)
EMBED_MAX_MEMBERS = 32
EMBED_MAX_EXCLUDE = 1024
EMBED_MAX_WEIGHT = 4.0


class EmbedQuery(ctypes.Structure):
    """mi355rec_embed_query_t; `size` is sizeof of this struct (72)."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("user", c_void_p), ("rows", c_void_p), ("audio", c_void_p),
                ("exclude_global", c_void_p), ("audio_row", c_int64), ("k", c_int32), ("n_exclude", c_int32), ("topn", c_int32),
                ("metric", c_int32), ("w_audio", c_float), ("w_embed", c_float)]


class EmbedResult(ctypes.Structure):
    """mi355rec_embed_result_t (32 bytes): out_score and out_count may be NULL."""
    _fields_ = [("size", c_uint32), ("reserved", c_uint32), ("out_idx", c_void_p), ("out_score", c_void_p), ("out_count", POINTER(c_int))]


class EmbedInfo(ctypes.Structure):
    """mi355rec_embed_info_t (56 bytes)."""
    _fields_ = [("size", c_uint32), ("dim", c_int32), ("rows", c_int64), ("device_bytes", c_int64), ("tile_rows", c_int32),
                ("grid", c_int32), ("device", c_int32), ("shards", c_int32), ("queries", c_int64), ("scores_launches", c_int64)]


EMBED_SIGNATURES = {
    "mi355rec_embed_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_create_node": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_destroy": (None, [c_void_p]),
    "mi355rec_embed_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_query": (c_int, [c_void_p, POINTER(EmbedQuery), POINTER(EmbedResult)]),
    "mi355rec_embed_scores": (c_int, [c_void_p, POINTER(EmbedQuery), c_void_p, c_void_p]),
    "mi355rec_embed_info": (c_int, [c_void_p, POINTER(EmbedInfo)]),
    "mi355rec_embed_enqueue_probe": (c_int, [c_void_p, c_void_p, c_void_p]),
}

_embed_lib = None


def embed_lib() -> ctypes.CDLL:
    """Load libmi355rec_embed.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share one
    copy of it and of the HIP runtime).  A missing library is an error: the hybrid scan has no fallback."""
    global _embed_lib
    if _embed_lib is None:
        lib()
        if not EMBED_LIB_PATH.exists():
            raise RuntimeError(f"{EMBED_LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(EMBED_LIB_PATH))
        for name, (restype, argtypes) in EMBED_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_lib = handle
    return _embed_lib


# ---- USER BATCHES: the second companion library libmi355rec_embed_batch.so (include/mi355rec_embed_batch.h), a third table ----
EMBED_BATCH_LIB_PATH = PKG / "libmi355rec_embed_batch.so"
EMBED_BATCH_MAX_USERS = 1024
EMBED_BATCH_MAX_TOPN = 128
EMBED_BATCH_MAX_EXCLUDE = 65536


class EmbedBatchQuery(ctypes.Structure):
    """mi355rec_embed_batch_query_t; `size` is sizeof of this struct (48)."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("users", c_void_p), ("exclude_global", c_void_p), ("exclude_offsets", c_void_p),
                ("n_users", c_int32), ("topn", c_int32), ("metric", c_int32), ("w_embed", c_float)]


class EmbedBatchResult(ctypes.Structure):
    """mi355rec_embed_batch_result_t (32 bytes): out_score and out_count may be NULL."""
    _fields_ = [("size", c_uint32), ("reserved", c_uint32), ("out_idx", c_void_p), ("out_score", c_void_p), ("out_count", c_void_p)]


class EmbedBatchInfo(ctypes.Structure):
    """mi355rec_embed_batch_info_t (56 bytes)."""
    _fields_ = [("size", c_uint32), ("dim", c_int32), ("rows", c_int64), ("device_bytes", c_int64), ("tile_rows", c_int32),
                ("grid", c_int32), ("device", c_int32), ("pass_users", c_int32), ("passes", c_int64), ("users_served", c_int64)]


EMBED_BATCH_SIGNATURES = {
    "mi355rec_embed_batch_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_batch_destroy": (None, [c_void_p]),
    "mi355rec_embed_batch_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_batch_query": (c_int, [c_void_p, POINTER(EmbedBatchQuery), POINTER(EmbedBatchResult)]),
    "mi355rec_embed_batch_info": (c_int, [c_void_p, POINTER(EmbedBatchInfo)]),
}

_embed_batch_libs = {}


def embed_batch_lib(path=None) -> ctypes.CDLL:
    """Load libmi355rec_embed_batch.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share
    one copy of it and of the HIP runtime).  A missing library is an error: the batch scan has no fallback.  `path`: a
    variant built by build.build_embed_batch(pass_users=P) (tools/run_embed_batch.py measures them)."""
    path = Path(path) if path else EMBED_BATCH_LIB_PATH
    if path not in _embed_batch_libs:
        lib()
        if not path.exists():
            raise RuntimeError(f"{path} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(path))
        for name, (restype, argtypes) in EMBED_BATCH_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_batch_libs[path] = handle
    return _embed_batch_libs[path]


class Mi355Error(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"mi355rec error {code}: {message}")
        self.code = code


def check(rc: int, handle=None) -> None:
    if rc == OK:
        return
    L = lib()
    msg = L.mi355rec_last_error(handle) if handle else L.mi355rec_last_global_error()
    raise Mi355Error(rc, (msg or b"").decode("utf-8", "replace"))


# ---- HALF-PRECISION EMBEDDING TABLES: the third companion library libmi355rec_embed_half.so
# (include/mi355rec_embed_half.h), a fourth table.  Queries and results are EmbedQuery / EmbedResult. ----
EMBED_HALF_LIB_PATH = PKG / "libmi355rec_embed_half.so"
EMBED_HALF_FP16, EMBED_HALF_BF16 = 0, 1


class EmbedHalfInfo(ctypes.Structure):
    """mi355rec_embed_half_info_t (64 bytes): EmbedInfo's fields, then the storage."""
    _fields_ = EmbedInfo._fields_ + [("storage", c_int32), ("reserved", c_int32)]


EMBED_HALF_SIGNATURES = {
    "mi355rec_embed_half_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_half_destroy": (None, [c_void_p]),
    "mi355rec_embed_half_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_half_query": (c_int, [c_void_p, POINTER(EmbedQuery), POINTER(EmbedResult)]),
    "mi355rec_embed_half_scores": (c_int, [c_void_p, POINTER(EmbedQuery), c_void_p, c_void_p]),
    "mi355rec_embed_half_info": (c_int, [c_void_p, POINTER(EmbedHalfInfo)]),
    "mi355rec_embed_half_enqueue_probe": (c_int, [c_void_p, c_void_p, c_void_p]),
}

_embed_half_lib = None


def embed_half_lib() -> ctypes.CDLL:
    """Load libmi355rec_embed_half.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share
    one copy of it and of the HIP runtime).  A missing library is an error: the half scan has no fallback."""
    global _embed_half_lib
    if _embed_half_lib is None:
        lib()
        if not EMBED_HALF_LIB_PATH.exists():
            raise RuntimeError(f"{EMBED_HALF_LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(EMBED_HALF_LIB_PATH))
        for name, (restype, argtypes) in EMBED_HALF_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_half_lib = handle
    return _embed_half_lib


# ---- RESTRICTED EMBEDDING REQUESTS: the fourth companion library libmi355rec_embed_sets.so
# (include/mi355rec_embed_sets.h), a fifth table.  Queries and results are EmbedQuery / EmbedResult. ----
EMBED_SETS_LIB_PATH = PKG / "libmi355rec_embed_sets.so"
EMBED_SETS_FP32 = -1   # `storage` of an fp32 table in EmbedSetsInfo


class EmbedSetsExt(ctypes.Structure):
    """mi355rec_embed_sets_ext_t (24 bytes): either set may be NULL."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("seen", c_void_p), ("only", c_void_p)]


class EmbedSetsInfo(ctypes.Structure):
    """mi355rec_embed_sets_info_t (88 bytes): EmbedHalfInfo's fields, then the cumulative counters."""
    _fields_ = EmbedHalfInfo._fields_ + [("tiles_total", c_int64), ("tiles_scored", c_int64), ("launches_skipped", c_int64)]


EMBED_SETS_SIGNATURES = {
    "mi355rec_embed_sets_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_sets_create_half": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_sets_destroy": (None, [c_void_p]),
    "mi355rec_embed_sets_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_sets_info": (c_int, [c_void_p, POINTER(EmbedSetsInfo)]),
    "mi355rec_embed_sets_rowset_create": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_void_p)]),
    "mi355rec_embed_sets_rowset_create_mask": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_void_p)]),
    "mi355rec_embed_sets_rowset_add": (c_int, [c_void_p, c_void_p, c_int64]),
    "mi355rec_embed_sets_rowset_count": (c_int64, [c_void_p]),
    "mi355rec_embed_sets_rowset_destroy": (None, [c_void_p]),
    "mi355rec_embed_sets_query": (c_int, [c_void_p, POINTER(EmbedQuery), POINTER(EmbedSetsExt), POINTER(EmbedResult)]),
}

_embed_sets_lib = None


def embed_sets_lib() -> ctypes.CDLL:
    """Load libmi355rec_embed_sets.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share
    one copy of it and of the HIP runtime).  A missing library is an error: the restricted scan has no fallback."""
    global _embed_sets_lib
    if _embed_sets_lib is None:
        lib()
        if not EMBED_SETS_LIB_PATH.exists():
            raise RuntimeError(f"{EMBED_SETS_LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(EMBED_SETS_LIB_PATH))
        for name, (restype, argtypes) in EMBED_SETS_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_sets_lib = handle
    return _embed_sets_lib


# ---- STREAMED EMBEDDING REQUESTS: the fifth companion library libmi355rec_embed_stream.so
# (include/mi355rec_embed_stream.h), a sixth table.  Every pointer named *_dev is device memory. ----
EMBED_STREAM_LIB_PATH = PKG / "libmi355rec_embed_stream.so"
EMBED_STREAM_FP32 = -1   # `storage` of an fp32 table; else EMBED_HALF_FP16 / EMBED_HALF_BF16
EMBED_STREAM_MAX_EXCLUDE = 1024
EMBED_STREAM_MAX_USERS = 1024
EMBED_STREAM_MAX_USERS_TOPN = 128


class EmbedStreamQuery(ctypes.Structure):
    """mi355rec_embed_stream_query_t; `size` is sizeof of this struct (64).  `audio` is 12 HOST floats."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("user_dev", c_void_p), ("audio", c_void_p), ("exclude_dev", c_void_p),
                ("audio_row", c_int64), ("n_exclude", c_int32), ("topn", c_int32), ("metric", c_int32), ("w_audio", c_float),
                ("w_embed", c_float), ("reserved", c_uint32)]


class EmbedStreamUsers(ctypes.Structure):
    """mi355rec_embed_stream_users_t; `size` is sizeof of this struct (48)."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("users_dev", c_void_p), ("exclude_dev", c_void_p), ("n_users", c_int32),
                ("topn", c_int32), ("exclude_len", c_int32), ("metric", c_int32), ("w_embed", c_float), ("reserved", c_uint32)]


class EmbedStreamResult(ctypes.Structure):
    """mi355rec_embed_stream_result_t (32 bytes): out_score_dev and out_count_dev may be NULL."""
    _fields_ = [("size", c_uint32), ("reserved", c_uint32), ("out_idx_dev", c_void_p), ("out_score_dev", c_void_p), ("out_count_dev", c_void_p)]


class EmbedStreamInfo(ctypes.Structure):
    """mi355rec_embed_stream_info_t (80 bytes)."""
    _fields_ = [("size", c_uint32), ("dim", c_int32), ("rows", c_int64), ("device_bytes", c_int64), ("tile_rows", c_int32),
                ("grid", c_int32), ("device", c_int32), ("storage", c_int32), ("table_dev", c_void_p), ("launches", c_int64),
                ("enqueues", c_int64), ("scores_launches", c_int64), ("pass_users", c_int32), ("borrowed", c_int32)]


EMBED_STREAM_SIGNATURES = {
    "mi355rec_embed_stream_create_device": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_stream_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_stream_destroy": (None, [c_void_p]),
    "mi355rec_embed_stream_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_stream_info": (c_int, [c_void_p, POINTER(EmbedStreamInfo)]),
    "mi355rec_embed_stream_enqueue_query": (c_int, [c_void_p, POINTER(EmbedStreamQuery), POINTER(EmbedStreamResult), c_void_p]),
    "mi355rec_embed_stream_enqueue_users": (c_int, [c_void_p, POINTER(EmbedStreamUsers), POINTER(EmbedStreamResult), c_void_p]),
}

_embed_stream_lib = None


def embed_stream_lib() -> ctypes.CDLL:
    """Load libmi355rec_embed_stream.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share
    one copy of it and of the HIP runtime).  A missing library is an error: the streamed requests have no fallback."""
    global _embed_stream_lib
    if _embed_stream_lib is None:
        lib()
        if not EMBED_STREAM_LIB_PATH.exists():
            raise RuntimeError(f"{EMBED_STREAM_LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(EMBED_STREAM_LIB_PATH))
        for name, (restype, argtypes) in EMBED_STREAM_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_stream_lib = handle
    return _embed_stream_lib


# ---- EMBEDDING CANDIDATE LISTS: the sixth companion library libmi355rec_embed_cand.so
# (include/mi355rec_embed_cand.h), a seventh table.  Every pointer named *_dev is device memory; a rank call's result is
# EmbedStreamResult. ----
EMBED_CAND_LIB_PATH = PKG / "libmi355rec_embed_cand.so"
EMBED_CAND_MAX = 1 << 20
EMBED_CAND_MAX_EXCLUDE = 1024


class EmbedCandQuery(ctypes.Structure):
    """mi355rec_embed_cand_query_t; `size` is sizeof of this struct (80).  `audio` is 12 HOST floats."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("user_dev", c_void_p), ("audio", c_void_p), ("candidates_dev", c_void_p),
                ("exclude_dev", c_void_p), ("audio_row", c_int64), ("n_candidates", c_int64), ("n_exclude", c_int32), ("topn", c_int32),
                ("metric", c_int32), ("w_audio", c_float), ("w_embed", c_float), ("reserved", c_uint32)]


class EmbedCandScores(ctypes.Structure):
    """mi355rec_embed_cand_scores_t (32 bytes): out_c_dev and out_flag_dev may be NULL."""
    _fields_ = [("size", c_uint32), ("reserved", c_uint32), ("out_v_dev", c_void_p), ("out_c_dev", c_void_p), ("out_flag_dev", c_void_p)]


class EmbedCandInfo(ctypes.Structure):
    """mi355rec_embed_cand_info_t (96 bytes): EmbedStreamInfo's fields, then the list's limit and the launches per call."""
    _fields_ = EmbedStreamInfo._fields_ + [("max_candidates", c_int32), ("rank_launches", c_int32), ("scores_call_launches", c_int32),
                                           ("reserved", c_int32)]


EMBED_CAND_SIGNATURES = {
    "mi355rec_embed_cand_create_device": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_cand_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_cand_destroy": (None, [c_void_p]),
    "mi355rec_embed_cand_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_cand_info": (c_int, [c_void_p, POINTER(EmbedCandInfo)]),
    "mi355rec_embed_cand_enqueue_rank": (c_int, [c_void_p, POINTER(EmbedCandQuery), POINTER(EmbedStreamResult), c_void_p]),
    "mi355rec_embed_cand_enqueue_scores": (c_int, [c_void_p, POINTER(EmbedCandQuery), POINTER(EmbedCandScores), c_void_p]),
}

_embed_cand_lib = None


def embed_cand_lib() -> ctypes.CDLL:
    """Load libmi355rec_embed_cand.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share
    one copy of it and of the HIP runtime).  A missing library is an error: the candidate lists have no fallback."""
    global _embed_cand_lib
    if _embed_cand_lib is None:
        lib()
        if not EMBED_CAND_LIB_PATH.exists():
            raise RuntimeError(f"{EMBED_CAND_LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(EMBED_CAND_LIB_PATH))
        for name, (restype, argtypes) in EMBED_CAND_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_cand_lib = handle
    return _embed_cand_lib


# ---- MULTI-INTEREST EMBEDDING REQUESTS: the seventh companion library libmi355rec_embed_multi.so
# (include/mi355rec_embed_multi.h), an eighth table.  Every pointer named *_dev is device memory. ----
EMBED_MULTI_LIB_PATH = PKG / "libmi355rec_embed_multi.so"
EMBED_MULTI_MAX_INTERESTS = 32
EMBED_MULTI_MAX_EXCLUDE = 1024


class EmbedMultiQuery(ctypes.Structure):
    """mi355rec_embed_multi_query_t; `size` is sizeof of this struct (72).  `audio` is 12 HOST floats."""
    _fields_ = [("size", c_uint32), ("flags", c_uint32), ("interests_dev", c_void_p), ("audio", c_void_p), ("exclude_dev", c_void_p),
                ("audio_row", c_int64), ("n_interests", c_int32), ("n_exclude", c_int32), ("topn", c_int32), ("metric", c_int32),
                ("w_audio", c_float), ("w_embed", c_float), ("reserved", c_uint64)]


class EmbedMultiResult(ctypes.Structure):
    """mi355rec_embed_multi_result_t (40 bytes): EmbedStreamResult's fields, then out_interest_dev; the last three may be NULL."""
    _fields_ = EmbedStreamResult._fields_ + [("out_interest_dev", c_void_p)]


class EmbedMultiInfo(ctypes.Structure):
    """mi355rec_embed_multi_info_t (96 bytes): EmbedStreamInfo's fields, then the interests' limit, the chunk width and the
    launches per call."""
    _fields_ = EmbedStreamInfo._fields_ + [("max_interests", c_int32), ("pass_interests", c_int32), ("query_launches", c_int32),
                                           ("reserved", c_int32)]


EMBED_MULTI_SIGNATURES = {
    "mi355rec_embed_multi_create_device": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_multi_create": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(c_void_p)]),
    "mi355rec_embed_multi_destroy": (None, [c_void_p]),
    "mi355rec_embed_multi_last_error": (c_char_p, [c_void_p]),
    "mi355rec_embed_multi_info": (c_int, [c_void_p, POINTER(EmbedMultiInfo)]),
    "mi355rec_embed_multi_enqueue_query": (c_int, [c_void_p, POINTER(EmbedMultiQuery), POINTER(EmbedMultiResult), c_void_p]),
}

_embed_multi_lib = None


def embed_multi_lib() -> ctypes.CDLL:
    """Load libmi355rec_embed_multi.so (it links against libmi355rec.so beside it; `lib()` is loaded first so that both share
    one copy of it and of the HIP runtime).  A missing library is an error: the multi-interest requests have no fallback."""
    global _embed_multi_lib
    if _embed_multi_lib is None:
        lib()
        if not EMBED_MULTI_LIB_PATH.exists():
            raise RuntimeError(f"{EMBED_MULTI_LIB_PATH} is missing: build it with `python -m spotify_recommender_amd.build`")
        handle = ctypes.CDLL(str(EMBED_MULTI_LIB_PATH))
        for name, (restype, argtypes) in EMBED_MULTI_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _embed_multi_lib = handle
    return _embed_multi_lib
