/*
 * mi355rec_diag.h — the rest of the C-ABI of libmi355rec.so: what a deployment does not need in order to serve queries.
 *
 * mi355rec.h is the core (create, query, enqueue, stream, lanes, the node handle: 30 entry points).  This header declares,
 * over the same handles and with the same conventions (plain pointers and sizes, 0 / negative codes, caller-owned buffers):
 *   - statistics and what the build is (mi355rec_stats*, _build_flags, _device_count, _last_global_error, _lane_status,
 *     _replica_counters, _batched_*, _sharded_info / _shard_stats / _stream_stats / _note / _rccl_ranks ...);
 *   - controls for A/B measurements and tests (mi355rec_create_ex flags, _set_replica, _rebuild_replica, _set_batch_path,
 *     _set_timing, _sharded_set_transport / _set_window / _set_window_mode / _set_replica);
 *   - the parity hook: the full score vector (mi355rec_scores*, the mirror of the private
 *     Recommender::calculateSimilarities, Recommender.h:114), and the probes (mi355rec_enqueue_stream_probe*);
 *   - the building blocks the multi-GPU layers are made of: queries by device pointer, mixed batches, the merge-only entry
 *     points (mi355rec_enqueue_merge_keys*), mi355rec_fetch_row, the explicit set-ups of the node handle;
 *   - LABELS, an extension beyond the reference (which lists "recommendations within genre" among its extensions only):
 *     rows carry an integer label (a genre id) and a query returns the top-N rows whose label is in a given set
 *     (mi355rec_set_labels, _query_row_topn_labels, _query_topn_labels, _label_counters and their node-handle twins);
 *   - PLAYLISTS, a further extension: the top-N rows by the mean of their scores against up to 32 songs, with an exclusion
 *     list (mi355rec_query_mean_topn, _query_playlist_topn, _playlist_counters and their node-handle twins);
 *   - FEATURE FILTERS, on the playlist calls: only rows whose audio features lie within given bounds are returned
 *     (mi355rec_query_mean_topn_where, _query_playlist_topn_where and their node-handle twins);
 *   - WEIGHTED PLAYLISTS: a signed weight per member, likes and dislikes
 *     (mi355rec_query_mean_topn_weighted, _query_playlist_topn_weighted and their node-handle twins);
 *   - DIVERSIFIED TOP-N: the weighted playlist call's top-`pool`, re-ranked by maximal marginal relevance over the 12
 *     features (mi355rec_query_mean_topn_diverse, _query_playlist_topn_diverse, their node-handle twins, mi355rec_fetch_rows);
 *   - group caps: "at most M results per artist" inside the same re-rank (mi355rec_set_groups, the _capped calls and their
 *     node-handle twins);
 *   - PLAYLIST REQUESTS: the whole playlist family as one call that takes a struct, and the only one that takes a label set
 *     (mi355rec_query_playlist_request and its node-handle twin);
 *   - ROW PRIORS: a per-row prior (popularity, freshness, a boost or a demotion) blended into the request's ranking value
 *     (mi355rec_set_priors, MI355REC_PQ_PRIOR and prior_weight of the request, and the node-handle twin);
 *   - DISTANCE REQUESTS: the nearest rows by Euclidean distance to up to 32 members, with the playlist request's exclusion
 *     list, feature filter and label set (mi355rec_query_distance_request and its node-handle twin);
 *   - FEATURE SCALES: 12 non-negative per-request factors that weigh or ignore features in the playlist and distance requests
 *     (mi355rec_query_playlist_request_scaled, mi355rec_query_distance_request_scaled and their node-handle twins);
 *   - ROW SETS: one bit per row, to leave out a listening history or to rank within a candidate set, passed to the playlist and
 *     distance requests in a self-sized struct of extras (mi355rec_rowset_*, mi355rec_query_*_request_ext and the node-handle twins);
 *   - ROW UPDATES: rows of the catalogue change in place and every route answers as a freshly created handle would
 *     (mi355rec_update_rows, _update_info, _replica_entries and the node-handle twin);
 *   - ANY-OF REQUESTS: the top-N rows by their best match among up to 32 members, with the matched member's index per result
 *     (mi355rec_query_anyof_request and its node-handle twin);
 *   - MANHATTAN REQUESTS: the nearest rows by L1 distance to up to 32 members, with the playlist request's exclusion list,
 *     feature filter, label set and row set (mi355rec_query_manhattan_request and its node-handle twin);
 *   - BOUNDED REQUESTS: only the rows at or above a score floor (or within a radius), and the exact number of such rows
 *     (mi355rec_query_bounded_request and its node-handle twin);
 *   - JACCARD REQUESTS: the top-N rows by weighted (Ruzicka) Jaccard similarity to up to 32 members, with the playlist request's
 *     exclusion list, feature filter, label set and row set (mi355rec_query_jaccard_request and its node-handle twin);
 *   - test hooks, compiled in only with -DMI355REC_TEST_HOOKS (spotify_recommender_amd/build.py builds
 *     libmi355rec_testhooks.so for tests/; the product library does not export them).
 */
#ifndef MI355REC_DIAG_H
#define MI355REC_DIAG_H

#include "mi355rec.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t rows;              /* rows held by this handle (local shard)      */
    int64_t row_base;          /* global index of local row 0                 */
    int32_t device;            /* HIP device ordinal                          */
    int32_t compute_units;     /* CUs of the device                           */
    int32_t grid_blocks;       /* resident workgroups of the streaming kernel */
    int32_t block_threads;
    int64_t bytes_per_query;   /* algorithmic bytes of one pass: rows * 48    */
    float last_scan_ms;        /* HIP-event time of the last timed scan       */
    float last_merge_ms;       /* HIP-event time of the last timed merge      */
    float last_pass_ms;        /* HIP-event time of the batched path's passes (mean of pass 1 and pass 2) */
    int32_t batched_grid_blocks; /* workgroups of a batched pass (0 before the first batched call) */
    float batched_margin;      /* error bound the fp16 pre-filter runs with: 1.0e-3 where the device keeps
                                  fp16 subnormals (checked on first use), 1.5e-3 otherwise */
    int64_t replica_bytes_per_query; /* algorithmic bytes of one pass over the fp16 replica: ceil(rows/2) * 48
                                        (0 = the handle has no replica)                     */
    int32_t replica_active;    /* 1 = single queries currently scan the replica (mi355rec_set_replica) */
    int32_t replica_grid_blocks; /* resident workgroups of the replica scan                 */
    float replica_build_ms;    /* device time of building the replica (once, at create)     */
    float replica_margin_single; /* error bound the replica pre-filters claim on this device: 1.0e-3 where the unit  */
    float replica_margin_multi;  /* demonstrably keeps fp16 subnormals (checked when the replica is built), else 1.5e-3:
                                    v_fma_mix_f32 (fp16 single-query scan) / the matrix core (multi-query pass)        */
    int64_t replica_single_bytes_per_query; /* algorithmic bytes of one SINGLE-query scan over the replica it currently
                                    uses: ceil(rows/4) * 48 over the 8-bit one, ceil(rows/2) * 48 over the fp16 one   */
    int32_t replica_single_row_bytes; /* 12 (8-bit replica), 24 (fp16 replica, MI355REC_REPLICA_FP16) or 0 (no replica)  */
    int32_t lone_fused_queries; /* synchronous single queries served by ONE scan launch that also merged and raised the
                                    completion word (8-bit replica, shards of >= 4 M rows), since create */
    /* WHICH ROUTE the work took, counted per launch since create (DESIGN.md has the table "AUTO route by rows, batch,
     * topn"; tests/test_gpu_routes.py asserts the counter that moves for each cell): */
    int64_t route_fp32;          /* single query: scan over the fp32 rows (48 B/row), plain or streamed             */
    int64_t route_fp16;          /* single query: scan over the fp16 replica (24 B/row; MI355REC_REPLICA_FP16)      */
    int64_t route_q8;            /* single query: scan over the 8-bit replica (12 B/row), plain or streamed         */
    int64_t route_q8_lone;       /* ... of a lone synchronous query that also merged and signalled (one launch)     */
    int64_t route_multi_fp32;    /* exact multi-query pass over the fp32 rows (<= 12 queries per pass)              */
    int64_t route_multi_fp16;    /* multi-query pass over the fp16 replica, fp16 matrix-core pre-filter (<= 32)     */
    int64_t route_multi_q8;      /* multi-query pass over the 8-bit replica, integer matrix-core pre-filter          */
    int64_t route_mfma_two_pass; /* chunks (<= 1024 queries) of the two-pass batched matrix-core path              */
    int64_t route_exact_queue;   /* queries that path handed to the exact scan on the device (reading it synchronises) */
    int32_t device_bytes_per_row; /* what the handle keeps resident per row: 48 (fp32) + 24 (fp16 replica) + 12 (8-bit) */
    int64_t stream_pair_launches; /* PAIRS of queued queries served by one pass over the 8-bit replica
                                     (mi355rec_set_stream_pairing); each pair still counts twice in route_q8, and a launch that
                                     served two pairs (below) adds 2 here */
    int64_t stream_group_launches; /* streamed launches that served TWO pairs (MI355REC_PAIRING_GROUPS) */
} mi355rec_stats_t;

/* What this build of the library was compiled with.  The product build returns 0.  The tools/ scripts build
 * instrumented copies under gpurun_out/ (never the product library): MI355REC_BUILD_EXPERIMENTS = environment knobs for
 * A/B runs and the routes that only exist for A/B (single queries over the fp16 replica: MI355REC_REPLICA_FP16; the
 * 8-bit front end of the multi-query pass: MI355REC_BATCH_Q8); MI355REC_BUILD_PHASE_CLOCK = per-workgroup phase stamps
 * (csrc/experiments.hip.h). */
#define MI355REC_BUILD_EXPERIMENTS 1
#define MI355REC_BUILD_PHASE_CLOCK 2
#define MI355REC_BUILD_TEST_HOOKS 4    /* mi355rec_debug_handoff is compiled in (libmi355rec_testhooks.so, the experiments build) */
int mi355rec_build_flags(void);

/* Number of visible HIP devices (0 when there is none / no driver). */
int mi355rec_device_count(void);

/* Thread-local text of the last error raised with no handle to attach it to
 * (e.g. a failed create); with a handle, use mi355rec_last_error. */
const char* mi355rec_last_global_error(void);

/* The same with FLAGS:
 *   MI355REC_CREATE_NO_REPLICA   the handle keeps the fp32 rows only: 48 B per row resident instead of 84 (no fp16 and no
 *                                8-bit copy is built, single queries scan the fp32 rows, batches of 13 and more take the
 *                                matrix-core path with rows from the fp32 matrix; mi355rec_set_replica(ON) is refused).
 *                                mi355rec_stats_t::device_bytes_per_row says what a handle holds. */
#define MI355REC_CREATE_NO_REPLICA 1
int mi355rec_create_ex(const float* feats_host, int64_t n, int dim, int device, int64_t row_base, int flags,
                       mi355rec_t** out);
int mi355rec_create_device_ex(const float* feats_dev, int64_t n, int dim, int device, int64_t row_base, int flags,
                              mi355rec_t** out);

/* THE fp16 REPLICA.  Next to the fp32 rows every handle keeps a second copy of
 * its shard that is only good enough to rule rows OUT: each row L2-normalised
 * and rounded to fp16, 24 B per row (+50 % device memory, built once inside
 * create; csrc/replica.hip.h).  A single query then streams 24 B per row
 * instead of 48: a row is skipped when its fp16 cosine is more than the derived
 * error bound (1.5e-3) below what the top-N needs; every row that is not
 * skipped is fetched from the fp32 matrix and scored by the reference's exact
 * chain, so ids, order and score bits are those of the fp32 scan and of
 * Recommender.cu:256-318.  Rows or queries the bound cannot be claimed for
 * (zero / tiny / huge / non-finite norms) are always scored exactly.
 *   AUTO (default): shards of >= 1 M rows scan the replica, smaller ones the
 *                   fp32 rows (a query is launch-bound there either way);
 *   OFF:            always the fp32 rows (the reference's own traffic, 48 B/row);
 *   ON:             always the replica;
 *   FP16:           as ON, with single queries on the fp16 replica (see below).
 * A handle with a replica holds two encodings of the normalised rows: fp16
 * (24 B/row, csrc/replica.hip.h: what the multi-query and batched passes
 * read, error bound 1.0e-3) and 8-bit (12 B/row, csrc/replica_q8.hip.h: what
 * single queries scan: signed bytes against a 16-bit query held as two int8 digits, six v_dot4_i32_i8 per
 * row and an integer candidate test; the bound is per query, l1(Q)/(254 S) + sqrt(12)/(2 S) + 3e-5 <= 0.0137, S = 32000).  Both are pre-filters in front of the same
 * exact chain; MI355REC_REPLICA_FP16 exists for A/B measurements.
 * The batched matrix-core path reads its rows from the replica too (they are
 * stored in exactly the form its MFMA operand wants) unless the mode is OFF.
 * The score vector (mi355rec_scores*), rounds of topn > 1024 after the first
 * and the exact multi-query pass always read the fp32 rows.
 * MI355REC_CREATE_NO_REPLICA (mi355rec_create_ex) creates a handle without either.
 * A replica is a SNAPSHOT: if the caller overwrites a borrowed matrix
 * (mi355rec_create_device) while the handle lives, it must call
 * mi355rec_rebuild_replica before the next query (synchronous). */
#define MI355REC_REPLICA_AUTO 0
#define MI355REC_REPLICA_OFF 1
#define MI355REC_REPLICA_ON 2
#define MI355REC_REPLICA_FP16 3
int mi355rec_set_replica(mi355rec_t* h, int mode);
int mi355rec_rebuild_replica(mi355rec_t* h);
/* Diagnostics, cumulative since create (synchronises the device): scans that
 * went over the replica, and rows those scans fetched from the fp32 matrix for
 * the exact chain.  Either pointer may be NULL. */
int mi355rec_replica_counters(mi355rec_t* h, int64_t* scans, int64_t* rescored_rows);

/* THE CUTOFF SAMPLE of a single query over the 8-bit replica (csrc/replica_q8.hip.h).  Every such query starts from a lower
 * bound of its topn-th score, taken from the exact scores of a sample of rows.
 *   STRIDED:  256 evenly spaced regions of 2048 rows (5 % of a 10 M-row shard, 6.3 MB per query), one value per 256 rows;
 *   BUCKETED: built once beside the replica — up to 1024 strided regions (a fifth of the rows) grouped by direction (the
 *             nearest of as many centroid rows) and kept as a contiguous copy in that order; a query reads the 32 regions
 *             whose buckets lie nearest to it (0.8 MB), one value per 64 rows.  +16 B per base row of device memory (32 MB
 *             at 10 M rows) and the build time mi355rec_bucket_sample_info reports.  INVALID_ARG where the handle has no
 *             such structure: shards whose 8-bit scan does not take exact sample values (under ~2.1 M rows on a 256-CU
 *             device) or created without a replica;
 *   AUTO (default): BUCKETED for topn <= 128 on shards of at least MI355REC_SAMPLE_AUTO_MIN_ROWS rows that have the
 *             structure, for the queries of a stream whose sample rides in the launch before; STRIDED otherwise — also for
 *             a query alone and the first of a stream, whose sample launch is on the critical path (5.4 us strided, 14.3
 *             bucketed) (measured, two lanes, top-100 / top-10 in us per query, strided -> bucketed:
 *             2.5 M rows 7.92 -> 8.0 / 7.22 -> 7.15, 4 M 8.35 -> 8.61 / 8.18 -> 8.44, 5 M 9.5 -> 9.23 / 9.2 -> 9.46,
 *             6 M 10.92 -> 10.35 / 10.35 -> 10.33, 7.5 M 13.17 -> 12.42 / 12.5 -> 12.03, 10 M 16.5 -> 15.75 / 16.17 -> 15.75).
 * Either way the sample only places the bound: results are those of the exact chain, bit for bit.  The mode belongs to the
 * handle (a lane has its own) and applies from the next query's sample on; a node handle's shards each decide for themselves. */
#define MI355REC_SAMPLE_AUTO 0
#define MI355REC_SAMPLE_STRIDED 1
#define MI355REC_SAMPLE_BUCKETED 2
#define MI355REC_SAMPLE_AUTO_MIN_ROWS 6000000
int mi355rec_set_sample(mi355rec_t* h, int mode);

/* PAIRS OF STREAMED QUERIES.  Two consecutive mi355rec_enqueue_*_streamed calls on a handle that both scan the 8-bit replica
 * and ask for the same topn <= 128 may be served by ONE pass over the replica: a tile is loaded once and scored against
 * both queries (csrc/replica_q8.hip.h, scan_q8_kernel_pair).  Everything per query — cutoff, candidates, exact re-scoring,
 * merge, keys — is what the one-query launch computes, bit for bit; only the bytes streamed per query halve.  The stream
 * then runs up to three calls behind instead of one (include/mi355rec.h).  A query without a partner (an odd tail at the
 * flush, another topn, a change of mi355rec_set_replica / _set_sample or a non-streamed call in between) takes the
 * one-query launch.  The two sample launches of the first pair of a stream take the sample a carried query would take under
 * mi355rec_set_sample(AUTO) (they are two calls ahead of the pair's launch, not on its critical path).
 *   AUTO (default): pairs on shards of at least MI355REC_PAIRING_AUTO_MIN_ROWS rows, groups (below) on shards of at least
 *                   MI355REC_GROUPS_AUTO_MIN_ROWS rows — there the first two pairs of a stream still go as pairs, and groups form
 *                   once a launch of the stream is under way (a short stream gains nothing from waiting for four queries);
 *   OFF:            never;
 *   ON:             pairs wherever the two queries qualify, never groups;
 *   GROUPS:         groups wherever four queries qualify, pairs otherwise.
 * The mode belongs to the handle; a lane inherits its parent's when it is created.  The shards of a node handle do not pair.
 *
 * GROUPS.  Two consecutive complete pairs with the same topn, replica mode and sample mode form a GROUP, and one launch
 * serves both pairs (scan_q8_kernel_pair, pairs == 2): every tile is scanned by two workgroups, one per pair, placed so that
 * on this hardware they share an XCD and run at nearly the same time — the tile one of them fetches from the Infinity Cache
 * the other finds in that XCD's L2.  Nothing but speed depends on the placement: no workgroup waits for another, and every
 * key is what the pair launch (and the one-query launch) computes, bit for bit.  The stream then runs up to SEVEN calls
 * behind for queries by row and by value: a waiting group of four and three queries of the group after it.  A query by
 * POINTER never waits longer than under pairs: it may complete a pair but closes its group, and while one waits for its
 * launch the group after it closes at one pair — its memory is read at most three calls later, as before.  A group with one
 * pair is the pair launch; a lone query is the one-query launch. */
#define MI355REC_PAIRING_AUTO 0
#define MI355REC_PAIRING_OFF 1
#define MI355REC_PAIRING_ON 2
#define MI355REC_PAIRING_GROUPS 3
#define MI355REC_PAIRING_AUTO_MIN_ROWS 2500000
/* From how many rows AUTO forms groups: the smallest measured size from which groups were not slower than pairs at top-10 and
 * top-100, for that size and every larger one measured (docs/LAB_NOTES.md, "two pairs per launch"): the smallest size measured. */
#define MI355REC_GROUPS_AUTO_MIN_ROWS 2500000
int mi355rec_set_stream_pairing(mi355rec_t* h, int mode);
typedef struct {
    int64_t base_rows;        /* rows of the base (0: the handle has no bucketed sample)                          */
    int32_t regions;          /* 2048-row regions of the ordered base                                            */
    int32_t centroids;        /* buckets: centroid i is local row i * centroid_stride + centroid_stride / 2      */
    int64_t bytes;            /* device memory of the structure                                                   */
    int64_t stride_rows;      /* base region g is local rows [g * stride_rows, g * stride_rows + 2048)            */
    int64_t centroid_stride;
    int32_t picks;            /* regions a query reads                                                            */
    int32_t mode;             /* MI355REC_SAMPLE_AUTO / _STRIDED / _BUCKETED as set                               */
    int32_t last_used;        /* _STRIDED or _BUCKETED: what the last query over the 8-bit replica took; 0: none yet */
    float build_ms;           /* host wall time of building it (inside create / mi355rec_rebuild_replica)         */
} mi355rec_bucket_sample_info_t;
int mi355rec_bucket_sample_info(const mi355rec_t* h, mi355rec_bucket_sample_info_t* out);
/* Copies the structure to the host: rows_out[regions * 2048] = the local row of every entry in (bucket, row) order (-1:
 * padding), region_tab_out[regions * 2] = the buckets of each region's first and last entry.  Either may be NULL.
 * INVALID_ARG where the handle has none.  Synchronises the handle's stream. */
int mi355rec_bucket_sample_rows(mi355rec_t* h, int32_t* rows_out, int32_t* region_tab_out);

/* What mi355rec_create_lane found when it chose the lane's stream: it times a small kernel on the parent's stream alone and
 * on both streams at once, and replaces the lane's stream (each new stream is bound to the next hardware queue) until the pair
 * runs side by side.  *stream_attempts = streams tried (0 on a handle that is not a lane); *overlaps_parent = 1 side by side,
 * 0 none of them did (the lane then buys nothing: use one handle), -1 not testable (under 10 000 rows). */
int mi355rec_lane_status(const mi355rec_t* h, int* stream_attempts, int* overlaps_parent);

int mi355rec_stats(const mi355rec_t* h, mi355rec_stats_t* out);
/* The same for a caller that may have been built against an EARLIER header: mi355rec_stats_t only ever grows at its end, and
 * this copies min(out_size, sizeof(mi355rec_stats_t)) bytes — a shorter struct gets the fields it knows, never an overrun.
 * Pass sizeof(mi355rec_stats_t) of the header you compiled with.  *written (may be NULL) = the bytes copied. */
int mi355rec_stats_sized(const mi355rec_t* h, void* out, size_t out_size, size_t* written);

/* ---- the score vector: the parity hook --------------------------------------- */

/* Replaces the private Recommender::calculateSimilarities(int, float*)
 * (Recommender.h:114, Recommender.cu:184-254): cosine of catalogue row
 * `local_row` against every local row, n floats written to host memory. */
int mi355rec_scores_row(mi355rec_t* h, int64_t local_row, float* out_host);

/* Same for an arbitrary query vector (12 floats, host). */
int mi355rec_scores(mi355rec_t* h, const float* query12, float* out_host);

/* Queries whose 12 floats ALREADY LIVE in memory this device can read: a resident
 * row of this handle, a row of ANOTHER shard on another GPU of the node (through
 * the peer mapping: how the row-sharded engine below hands a catalogue row to every
 * shard without a host round trip), a staged vector in mapped host memory.  The
 * kernels fetch them with scalar loads when they start; the 48 bytes must not
 * change until the query has completed.  mi355rec_row_ptr returns where a resident
 * row lives (valid for the lifetime of the handle).  Otherwise as
 * mi355rec_enqueue_query_keys / _query_keys_streamed; out_idx_dev / out_score_dev
 * may be NULL. */
int mi355rec_row_ptr(mi355rec_t* h, int64_t local_row, const float** out_dev);
int mi355rec_enqueue_ptr_keys(mi355rec_t* h, const float* query12_dev, int64_t exclude_global, int topn,
                              mi355rec_key_t* out_keys_dev, int64_t* out_idx_dev, float* out_score_dev,
                              void* stream);
int mi355rec_enqueue_ptr_keys_streamed(mi355rec_t* h, const float* query12_dev, int64_t exclude_global,
                                       int topn, mi355rec_key_t* out_keys_dev, void* stream);
/* (The streamed form reads query12_dev when its launches run: by the work enqueued up to three streamed calls after this
 * one, or by the flush — under pairs and under groups alike.  The memory must stay as it is until that work has completed.) */

/* A batch whose queries are vectors (queries[i*12 ..], host) and / or POINTERS to 12 floats in
 * device-readable memory (query_ptrs_dev[i] != NULL wins; either array may be NULL when the other
 * covers every query): what a window of the row-sharded stream hands to every shard.  With a
 * replica (mi355rec_batch_pointers_ok: shard of >= 65536 rows, topn <= 128, sample large enough)
 * the batch goes in multi-query passes over the replica, up to 32 queries per pass
 * (csrc/replica_multi.hip.h); otherwise one scan per query.  topn <= 1024. */
int mi355rec_batch_pointers_ok(const mi355rec_t* h, int topn);
int mi355rec_enqueue_batch_mixed_keys(mi355rec_t* h, const float* queries, const float* const* query_ptrs_dev,
                                      const int64_t* exclude_global, int batch, int topn,
                                      mi355rec_key_t* out_keys_dev, void* stream);
/* ... and as a stream of batches (mi355rec_enqueue_batch_keys_streamed's deferred completion). */
int mi355rec_enqueue_batch_mixed_keys_streamed(mi355rec_t* h, const float* queries, const float* const* query_ptrs_dev,
                                               const int64_t* exclude_global, int batch, int topn,
                                               mi355rec_key_t* out_keys_dev, void* stream);

/* How batches (topn <= 128) are served.  AUTO: up to 12 queries as one
 * multi-query pass; 13 and more on shards of >= 65536 rows through the batched
 * path: two passes over the shard per chunk of up to 1024 queries, in which a
 * conservative fp16 pre-filter on the matrix cores (v_mfma_f32_32x32x16_f16 on
 * L2-normalised rows x queries, error bound 1.0e-3 derived in
 * csrc/batched.hip.h) selects a few hundred candidate rows per query that are
 * then scored with the exact fp32 chain — results stay bit-identical to the
 * single-query path.  Queries the bound cannot be claimed for (tiny / huge /
 * non-finite norms, fewer than topn+1 clearly positive groups, more candidates
 * than a query's list holds: about rows / 64, at most 65536) are served by the
 * exact multi-query scan inside the same call.
 * MULTI / MFMA force one path (tests, A/B measurements).  The first batched
 * call allocates the path's scratch (~0.3 GB + the candidate lists, 8 ... 256
 * MB); later calls allocate nothing. */
#define MI355REC_BATCH_AUTO 0
#define MI355REC_BATCH_MULTI 1
#define MI355REC_BATCH_MFMA 2
#define MI355REC_BATCH_HALF 3   /* multi-query passes (<= 32 queries each) with rows from the fp16 replica, whatever the count */
#define MI355REC_BATCH_Q8 4     /* the same passes with rows from the 8-bit replica (integer matrix core, candidates re-checked
                                   against their fp16 rows): half the bytes, but 3.7 us per query of a pass instead of 0.85 —
                                   AUTO takes it for passes of one or two queries only */
/* ... and how much of pass 2 the tile maxima of pass 1 saved in that chunk: the (64-row tile, 32-query block) pairs whose
 * MFMAs pass 2 ran, out of all of them (equal when the chunk ran without tile maxima: fewer than 512 queries, no replica,
 * MI355REC_BATCH_MFMA_NOSKIP).  Synchronises the device. */
int mi355rec_batched_pass2_pairs(mi355rec_t* h, int64_t* pairs_done, int64_t* pairs_total);

#define MI355REC_BATCH_MFMA_NOSKIP 5   /* MFMA, but pass 2 looks at every (tile, query block) pair instead of skipping those the
                                   maxima pass 1 left behind rule out (csrc/batched.hip.h, kTileMax): A/B measurements, tests */
int mi355rec_set_batch_path(mi355rec_t* h, int path);

/* Diagnostics of the LAST chunk (<= 1024 queries) the batched path served on
 * this handle (synchronises the device): special rows listed, queries handed to
 * the exact multi-query scan, and the candidates the pre-filter let through
 * (total and per-query maximum, over the queries it served itself).  Any
 * pointer may be NULL. */
int mi355rec_batched_last_counters(mi355rec_t* h, int32_t* special_rows,
                                   int32_t* queued_queries, int64_t* candidates_total,
                                   int32_t* candidates_max);

/* Merge `n_lists` lists of `list_len` packed keys each (each sorted
 * descending, 0-padded — e.g. the all-gathered per-rank outputs of
 * mi355rec_enqueue_*_keys) into the global best `topn` keys (sorted
 * descending, 0-padded), and optionally unpack them.  out_idx_dev /
 * out_score_dev may be NULL.  Unused idx slots are -1.
 * topn <= MI355REC_MAX_TOPN_FAST here. */
int mi355rec_enqueue_merge_keys(mi355rec_t* h, const mi355rec_key_t* lists_dev,
                                int n_lists, int list_len, int topn,
                                mi355rec_key_t* out_keys_dev,
                                int64_t* out_idx_dev, float* out_score_dev,
                                void* stream);

/* Batched merge: query b's list l starts at lists_dev + b*query_stride +
 * l*list_stride (in keys).  [rank][query][key] data straight out of an
 * all-gather of per-rank batch results is list_stride = batch*topn,
 * query_stride = topn.  Outputs are batch x topn. */
int mi355rec_enqueue_merge_keys_batch(mi355rec_t* h, const mi355rec_key_t* lists_dev,
                                      int n_lists, int list_len, int64_t list_stride,
                                      int64_t query_stride, int batch, int topn,
                                      mi355rec_key_t* out_keys_dev, int64_t* out_idx_dev,
                                      float* out_score_dev, void* stream);

/* Full score vector into device memory (local_row >= 0: query = that row and
 * query12 is ignored; local_row < 0: query12 is used). */
int mi355rec_enqueue_scores(mi355rec_t* h, int64_t local_row,
                            const float* query12, float* out_scores_dev,
                            void* stream);

/* Plain read-only streaming kernel over the same matrix (the achievable-HBM
 * ceiling probe of SURVEY.md §8(d)); writes one checksum word per workgroup
 * to sink_dev (>= compute_units uint32). */
int mi355rec_enqueue_stream_probe(mi355rec_t* h, uint32_t* sink_dev, void* stream);
/* The same plain read over ANOTHER buffer of the handle, so that a kernel's rate can be held against the read ceiling of
 * the buffer it actually streams, in the memory that buffer actually lives in (a 120 MB 8-bit replica sits in the 256 MiB
 * Infinity Cache; the 480 MB fp32 matrix does not): MI355REC_PROBE_FP32_ROWS (what mi355rec_enqueue_stream_probe
 * reads), _FP16_REPLICA (24 B/row: the multi-query and batched passes), _Q8_REPLICA (12 B/row: single queries).
 * MI355REC_ERR_INVALID_ARG when the handle has no such buffer. */
#define MI355REC_PROBE_FP32_ROWS 0
#define MI355REC_PROBE_FP16_REPLICA 1
#define MI355REC_PROBE_Q8_REPLICA 2
int mi355rec_enqueue_stream_probe_of(mi355rec_t* h, int which, uint32_t* sink_dev, void* stream);

/* Brackets the following scan / merge launches with HIP events on their stream
 * so that mi355rec_stats reports last_scan_ms / last_merge_ms (averages over
 * the recorded launches; reading them synchronises the events).  enabled = 0
 * disables, 1 times every launch, k > 1 times every k-th launch of each kind
 * (an event pair costs a few microseconds of stream time). */
int mi355rec_set_timing(mi355rec_t* h, int enabled);

/* The 12 features of one resident row, copied back to the host (48 bytes). */
int mi355rec_fetch_row(mi355rec_t* h, int64_t local_row, float* out12_host);
/* The features of `count` resident rows, copied back to the host in the order asked (count x 12 floats): ids in any order,
 * duplicates allowed.  One gather launch and one copy per 1024 rows, not a copy per row. */
int mi355rec_fetch_rows(mi355rec_t* h, const int64_t* local_rows, int64_t count, float* out_host);

/* ---- the node handle (mi355rec.h: mi355rec_create_placed): set-up variants, controls, statistics ---- */

/* n_devices = 0: the library decides (mi355rec_auto_shards: as many devices as keep at least 4 M rows per
 * shard — a smaller shard is launch-bound and every shard adds to the exchange; 1 device up to 7.9 M rows, 2 at
 * 10 M, all 8 of a node from 32 M rows on); otherwise devices 0 .. n_devices-1.  `feats_host` is the whole
 * row-major n x 12 matrix; each device receives its own block only.
 * (= mi355rec_create_placed(feats, n, dim, NULL, n_devices, MI355REC_PLACEMENT_SHARDED, out).) */
int mi355rec_create_sharded(const float* feats_host, int64_t n, int dim, int n_devices,
                            mi355rec_sharded_t** out);
int mi355rec_auto_shards(int64_t n, int visible_devices);       /* the size-aware default; 0 without a device */
int mi355rec_sharded_placement(const mi355rec_sharded_t* h);    /* MI355REC_PLACEMENT_SHARDED, _REPLICATED or _CPU */

/* Explicit placement: shard r on device devices[r].  A device may appear more
 * than once (virtual shards: several shards of one GPU; how the orchestration is
 * exercised on a one-GPU box) — the RCCL transport then refuses, the peer
 * transport degenerates to stores into local memory. */
int mi355rec_create_sharded_on(const float* feats_host, int64_t n, int dim, const int* devices,
                               int n_shards, mi355rec_sharded_t** out);

int mi355rec_sharded_set_transport(mi355rec_sharded_t* h, int transport);

/* Any out pointer may be NULL; devices_out / shard_rows_out need n_shards slots. */
int mi355rec_sharded_info(const mi355rec_sharded_t* h, int* n_shards, int* transport,
                          int64_t* rows, int* devices_out, int64_t* shard_rows_out);

/* Per-shard diagnostics: mi355rec_set_timing on every shard's engine, and the
 * mi355rec_stats of one shard (kernel event times, grid geometry, replica state). */
int mi355rec_sharded_set_timing(mi355rec_sharded_t* h, int enabled);
int mi355rec_sharded_shard_stats(const mi355rec_sharded_t* h, int shard, mi355rec_stats_t* out);
/* mi355rec_set_replica on every shard (AUTO / OFF / ON); flushes an open stream window first. */
int mi355rec_sharded_set_replica(mi355rec_sharded_t* h, int mode);

/* 1 when queries by row are read by every shard straight from the owning shard's
 * memory (all-pairs peer access, verified against the by-value path when the handle
 * was created), 0 when the row is fetched to the host once per query.  The note says
 * why a fast path was switched off ("" when none was). */
int mi355rec_sharded_rows_by_pointer(const mi355rec_sharded_t* h);
const char* mi355rec_sharded_note(const mi355rec_sharded_t* h);

/* As mi355rec_scores_row, with a GLOBAL row index. */
int mi355rec_sharded_scores_row(mi355rec_sharded_t* h, int64_t global_row, float* out_host);

int mi355rec_sharded_set_window(mi355rec_sharded_t* h, int window);   /* default 16; flushes an open window */
/* How a window runs on the shards.  batched = 1 (default): where every shard can take a batch in
 * multi-query passes over its fp16 replica (shards of >= 65536 rows, topn <= 128, window >= 2:
 * mi355rec_batch_pointers_ok) the queries of a window are collected on the host and reach every shard
 * in ONE mi355rec_enqueue_batch_mixed_keys call when the window closes — three launches per shard per
 * WINDOW and one pass over the shard per 32 queries, at the price that a query only starts when its
 * window closes (or at the flush).  batched = 0, or shards that cannot: one streamed scan launch per
 * shard per QUERY, as described above. */
int mi355rec_sharded_set_window_mode(mi355rec_sharded_t* h, int batched);
/* Host-side cost accounting of the stream (cumulative since create): queries
 * enqueued, exchanges issued, and the wall-clock nanoseconds the enqueue / flush
 * calls themselves took on the host thread.  Any pointer may be NULL. */
int mi355rec_sharded_stream_stats(const mi355rec_sharded_t* h, int64_t* queries, int64_t* exchanges,
                                  int64_t* host_ns);

/* What RCCL itself reports about the communicators of MI355REC_TRANSPORT_RCCL: *comms = communicators the handle holds (one
 * per shard; 0 until that transport has been used), *ranks = ncclCommCount of the first, *ranks_agree = 1 when every
 * communicator reports the same count and its own shard index as its rank (ncclCommUserRank).  bench.py --gpus N puts these
 * in its line, so that a first run on a real node answers "did RCCL see N ranks" by itself.  Any pointer may be NULL. */
int mi355rec_sharded_rccl_ranks(const mi355rec_sharded_t* h, int* comms, int* ranks, int* ranks_agree);

/* LABELS (an extension beyond the reference): label-filtered top-N.
 * Every row of a handle may carry a label in [0, MI355REC_MAX_LABELS) — a genre id, or any category the caller chooses —
 * or -1 (unlabelled: never returned by a filtered query).  mi355rec_set_labels builds a copy of the shard's fp32 rows
 * grouped by label (labels ascending, rows stable inside a label, unlabelled rows last; +54 B per row of device memory:
 * the 48-B row, its 4-B original index and its label in row order as int16, what PLAYLIST REQUESTS read) and the label offsets.  It gathers the rows to the host, sorts them there
 * and uploads the copy: a one-time cost, O(n), paid by this call.  Calling it again replaces the labels; labels_host ==
 * NULL drops them; n must be the handle's row count.  A failure (out of memory, a HIP error) leaves the previous labels in
 * place.  A handle that has lanes (mi355rec_create_lane) refuses it (INVALID_ARG): the labels are shared by the group, and
 * a lane made afterwards shares them without a copy.
 * A filtered query has the arithmetic, canonical order (score descending, then row ascending, -0.0 reported as +0.0)
 * and exclusion of mi355rec_query_row_topn / _query_topn, restricted to the rows whose label is in labels[0..n_labels)
 * (duplicates allowed): count = min(topn, |selected rows| - [the excluded row is selected]), the rest padded with -1 / 0;
 * a set whose labels hold no rows answers count 0.  INVALID_ARG (with a message) for n_labels <= 0, a label outside
 * [0, MI355REC_MAX_LABELS) and a handle without labels.  One launch per query (per round of 1024 above topn 1024) scans
 * only the selected labels' rows (csrc/labels.hip.h), then the merge.  No asynchronous, streamed or windowed variant.
 * mi355rec_label_counters: filtered queries since create, and the rows their launches scanned (whole tiles of 512 rows
 * per selected label).  Either pointer may be NULL.
 * Node handle: one shard forwards; a replicated placement gives the labels to every replica and a query to one of them;
 * a row-sharded one gives each shard its slice, runs a query on every shard (by value, the query row excluded by its
 * global index) and merges the per-shard lists on the host (exact).  If any shard fails, the labels are dropped on
 * every shard.  The CPU backend (hosts without a device) serves the same calls. */
#define MI355REC_MAX_LABELS 1024
int mi355rec_set_labels(mi355rec_t* h, const int32_t* labels_host, int64_t n);
int mi355rec_query_row_topn_labels(mi355rec_t* h, int64_t local_row, const int32_t* labels, int n_labels, int topn,
                                   int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_query_topn_labels(mi355rec_t* h, const float* query12, int64_t exclude_global, const int32_t* labels,
                               int n_labels, int topn, int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_label_counters(const mi355rec_t* h, int64_t* queries, int64_t* rows_scanned);
int mi355rec_sharded_set_labels(mi355rec_sharded_t* h, const int32_t* labels_host, int64_t n);
int mi355rec_sharded_query_row_topn_labels(mi355rec_sharded_t* h, int64_t global_row, const int32_t* labels, int n_labels,
                                           int topn, int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_sharded_query_topn_labels(mi355rec_sharded_t* h, const float* query12, int64_t exclude_global,
                                       const int32_t* labels, int n_labels, int topn, int64_t* out_idx, float* out_score,
                                       int* out_count);

/* PLAYLISTS (an extension beyond the reference): "what goes with this playlist".
 * Members are K query vectors q_0 .. q_{K-1}, 1 <= K <= MI355REC_MAX_PLAYLIST, given by value (queries: K x 12 floats on the
 * host) or as rows of the catalogue; duplicates count with their multiplicity.  Every row x scores
 *     score(x) = fl( fl(...fl(c_0 + c_1) + ... + c_{K-1}) / (float)K ),   c_k = the score mi355rec_query_topn gives x for q_k,
 * summed in fp32 in member order with one IEEE divide: for K = 1 exactly the single query's score.  The excluded set is
 * the union of the member rows (by-row calls) and exclude_global[0..n_exclude) (global row ids, any order, duplicates
 * allowed, n_exclude <= MI355REC_MAX_EXCLUDE).  Results are in the canonical order of every other route (score
 * descending, then row ascending, -0.0 reported as +0.0); count = min(topn, rows - |distinct excluded rows|), the rest
 * padded with -1 / 0.  Version 1 answers in ONE round: topn <= 1024.
 * INVALID_ARG (with a message) for K outside [1, 32], topn <= 0 or > 1024, a member row outside the catalogue (local
 * rows of the handle; global rows of a node handle), an excluded id < 0 (on a node handle: outside the catalogue),
 * n_exclude outside [0, 1024] and a NULL list with n_exclude > 0.  On a single handle an excluded id of another shard's
 * rows matches nothing.
 * Synchronous, like the label calls: one launch (csrc/playlist.hip.h; csrc/playlist_cut.hip.h: a pre-filter over the 8-bit replica with a derived
 * error bound, K exact chains per surviving row) and the merge.  No set-up: lanes and node handles answer at once.
 * mi355rec_playlist_counters: playlist queries since create, and the rows whose K exact chains were computed (the
 * pre-filter's survivors, the rows of each workgroup's starting bound, every row where the pre-filter is off).  Either
 * pointer may be NULL.
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches the member rows
 * (mi355rec_fetch_row), asks every shard by value with the whole exclusion list (the members' global rows added) and
 * merges the per-shard lists on the host (exact).  The CPU backend (hosts without a device) serves the same calls. */
#define MI355REC_MAX_PLAYLIST 32
#define MI355REC_MAX_EXCLUDE 1024
int mi355rec_query_mean_topn(mi355rec_t* h, const float* queries, int k, const int64_t* exclude_global, int n_exclude, int topn,
                             int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_query_playlist_topn(mi355rec_t* h, const int64_t* local_rows, int k, const int64_t* exclude_global, int n_exclude,
                                 int topn, int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_playlist_counters(const mi355rec_t* h, int64_t* queries, int64_t* rows_exact);
int mi355rec_sharded_query_mean_topn(mi355rec_sharded_t* h, const float* queries, int k, const int64_t* exclude_global,
                                     int n_exclude, int topn, int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_sharded_query_playlist_topn(mi355rec_sharded_t* h, const int64_t* global_rows, int k, const int64_t* exclude_global,
                                         int n_exclude, int topn, int64_t* out_idx, float* out_score, int* out_count);

/* FEATURE FILTERS (an extension beyond the reference): "songs like these, but only high-energy".
 * A row x passes the filter iff, for every feature j whose bit is set in `active` (j < MI355REC_DIM),
 *     lo[j] <= x[j] && x[j] <= hi[j]      (IEEE compares on the stored fp32 feature)
 * so a NaN feature fails any active bound, -0.0 equals +0.0 and +-inf bounds are allowed.  The features are the catalogue's
 * 12 columns (Song.h: danceability, energy, key, loudness, mode, speechiness, acousticness, instrumentalness, liveness,
 * valence, tempo, genre id), in whatever units the matrix holds (the drop-in's songs_data.bin: min-max normalised to [0, 1]).
 * The _where calls are the playlist calls above with a filter: they return the top-N of the rows that pass, are not excluded
 * and are not members (by-row calls), with the playlist call's scores bit for bit and the canonical order;
 * count = min(topn, |admissible rows|), the rest padded with -1 / 0; topn <= 1024.  A filtered SINGLE query is the K = 1
 * form (a one-song playlist is exactly the single query): there are no separate single-query entry points.
 * A NULL filter or active == 0 is exactly the unfiltered call (same results, same launch).
 * INVALID_ARG (with a message): the playlist calls' cases, and a bit of `active` at or above MI355REC_DIM, a NaN bound or
 * lo[j] > hi[j] on an active feature.
 * mi355rec_playlist_counters counts filtered calls too; their rows_exact is every row read from the fp32 matrix, the rows
 * the filter then rejected included (rejected rows never take the K chains).
 * Device: the filter is tested inside playlist_scan_kernel on each fp32 row it reads (csrc/playlist.hip.h, "FEATURE
 * FILTER"), with no set-up: lanes and node handles answer at once.  Node handles as for the playlist calls: a row-sharded
 * one asks every shard by value with the filter and merges on the host.  The CPU backend serves the same calls. */
typedef struct {
    uint32_t active; /* bit j (j < 12): feature j is constrained; higher bits: INVALID_ARG */
    float lo[12];    /* a row x passes iff, for every active j,  lo[j] <= x[j] && x[j] <= hi[j]  (IEEE compares) */
    float hi[12];
} mi355rec_filter_t;
int mi355rec_query_mean_topn_where(mi355rec_t* h, const float* queries, int k, const int64_t* exclude_global, int n_exclude,
                                   const mi355rec_filter_t* filter, int topn, int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_query_playlist_topn_where(mi355rec_t* h, const int64_t* local_rows, int k, const int64_t* exclude_global,
                                       int n_exclude, const mi355rec_filter_t* filter, int topn, int64_t* out_idx, float* out_score,
                                       int* out_count);
int mi355rec_sharded_query_mean_topn_where(mi355rec_sharded_t* h, const float* queries, int k, const int64_t* exclude_global,
                                           int n_exclude, const mi355rec_filter_t* filter, int topn, int64_t* out_idx,
                                           float* out_score, int* out_count);
int mi355rec_sharded_query_playlist_topn_where(mi355rec_sharded_t* h, const int64_t* global_rows, int k,
                                               const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                               int topn, int64_t* out_idx, float* out_score, int* out_count);

/* WEIGHTED PLAYLISTS (an extension beyond the reference): "more like these, less like those", recency weights, one seed
 * song coloured by others.  The _weighted calls are the _where calls above plus `weights`: k floats on the host, one per
 * member, of any sign.  With c_k the score mi355rec_query_topn gives a row for member k (bit for bit),
 *     W        = fl(...fl(|w_0| + |w_1|) + ... + |w_{k-1}|)                                   (fp32, member order)
 *     score(x) = fl( fl(...fl( fl(w_0 c_0) + fl(w_1 c_1) ) + ... + fl(w_{k-1} c_{k-1}) ) / W )
 * in fp32, member order, multiply then add (never fused), one IEEE divide; scores lie in [-1, 1].  Everything else is the
 * playlist contract: canonical order (score descending, then row ascending, -0.0 reported as +0.0), member rows excluded
 * on by-row calls WHATEVER their weight (zero and negative weights too), up to MI355REC_MAX_EXCLUDE further ids, the
 * optional filter, count = min(topn, |admissible rows|), topn <= 1024.
 * Two identities follow: all weights 1.0f give the playlist call's result bit for bit (fl(1 c) = c, W = k exactly), and
 * scaling every weight by one power of two changes neither ids nor score bits while nothing over- or underflows.
 * weights == NULL is exactly the _where call with the same other arguments (same results, same launch).
 * INVALID_ARG (with a message): the playlist and filter cases, and a weight that is NaN or infinite, |w_k| > 1e6, or
 * W < 1e-6 (all weights zero included).  mi355rec_playlist_counters counts weighted calls too.
 * Device: the same playlist_scan_kernel launch (csrc/playlist.hip.h); the 8-bit pre-filter (csrc/playlist_cut.hip.h, "PLAIN") works on the weighted mean
 * direction u = (sum_k w_k q_k / |q_k|) / W and switches itself off when |u| < 1e-3 (likes and dislikes that cancel): every
 * row then takes the k exact chains.  Dislikes shrink |u| and let fewer rows be ruled out.  Node handles
 * as for the playlist calls; the CPU backend serves the same calls with the same arithmetic. */
int mi355rec_query_mean_topn_weighted(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                      int n_exclude, const mi355rec_filter_t* filter, int topn, int64_t* out_idx, float* out_score,
                                      int* out_count);
int mi355rec_query_playlist_topn_weighted(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                          const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, int topn,
                                          int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_sharded_query_mean_topn_weighted(mi355rec_sharded_t* h, const float* queries, const float* weights, int k,
                                              const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                              int topn, int64_t* out_idx, float* out_score, int* out_count);
int mi355rec_sharded_query_playlist_topn_weighted(mi355rec_sharded_t* h, const int64_t* global_rows, const float* weights, int k,
                                                  const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                                  int topn, int64_t* out_idx, float* out_score, int* out_count);

/* DIVERSIFIED TOP-N (an extension beyond the reference): results that are spread out, not ten variations of one song.
 * Maximal marginal relevance over the data the handle already holds, the 12 features.  The _diverse calls are the _weighted
 * calls above (weights and filter may be NULL; a single query is k = 1) plus `lambda`, `pool` and `out_mmr`:
 *   - the POOL is what the _weighted call returns for the same members, weights, exclusion list and filter with topn = pool:
 *     P' = min(pool, |admissible rows|) rows in canonical order; pool row i has relevance rel_i, that call's score bit for bit;
 *   - c(i, p) is the score mi355rec_query_topn gives row i (the scanned row) for a query vector equal to row p's 12 stored
 *     features: the exact sequential chain, never NaN;
 *   - mu = fl(1 - lambda), once; pen_i starts at +0.0f; after a row p is picked every unpicked row i takes
 *     pen_i = c(i, p) if c(i, p) > pen_i (IEEE >), else keeps pen_i;
 *   - mmr_i = fl( fl(lambda rel_i) - fl(mu pen_i) ): fp32, multiply, round, subtract, round, never fused;
 *   - each step picks the unpicked pool row with the largest mmr_i (IEEE >); a tie goes to the earlier pool position (the
 *     higher relevance, then the lower row id), so the first pick is pool row 0; min(topn, P') picks.
 * out_idx[t] is the row picked at step t (pick order), out_score[t] its relevance (the similarity a user understands; -0.0
 * reported as +0.0), out_mmr[t] (may be NULL) the mmr value it was picked with; padding -1 / 0 / 0;
 * *out_count = min(topn, P').
 * Identities, bit for bit: lambda = 1.0f gives the _weighted call's top-N for any pool >= topn, with out_mmr == out_score;
 * pool == topn gives a permutation of the _weighted call's top-N; the result does not depend on shard count, placement, lane
 * or replica mode.
 * INVALID_ARG (with a message): every case of the weighted, filter and playlist calls; lambda NaN or outside [0, 1];
 * pool < topn or pool > MI355REC_MAX_TOPN_FAST (so topn <= 1024).  mi355rec_playlist_counters counts these calls too.
 * Device: the playlist scan and its merge leave the pool's keys on the device; mmr_rerank_kernel (csrc/diverse.hip.h), one
 * workgroup with the pool's rows in LDS, picks serially and stores the results into the handle's pinned result slots with
 * the completion word: one wait per call, no set-up, lanes and node handles answer at once.
 * Node handle: one shard forwards, a replicated placement asks one replica; a row-sharded one takes the pool from its
 * weighted path (per-shard lists merged on the host), gathers the pool rows' features from their owning shards
 * (mi355rec_fetch_rows) and runs the same kernel on its first shard's device over the pool passed by value.  The CPU
 * backend serves the same calls with the same arithmetic. */
int mi355rec_query_mean_topn_diverse(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                     int n_exclude, const mi355rec_filter_t* filter, float lambda, int pool, int topn, int64_t* out_idx,
                                     float* out_score, float* out_mmr, int* out_count);
int mi355rec_query_playlist_topn_diverse(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                         const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, float lambda,
                                         int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr, int* out_count);
int mi355rec_sharded_query_mean_topn_diverse(mi355rec_sharded_t* h, const float* queries, const float* weights, int k,
                                             const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                             float lambda, int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr,
                                             int* out_count);
int mi355rec_sharded_query_playlist_topn_diverse(mi355rec_sharded_t* h, const int64_t* global_rows, const float* weights, int k,
                                                 const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                                 float lambda, int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr,
                                                 int* out_count);

/* GROUP CAPS (an extension beyond the reference): "at most two per artist".
 * mi355rec_set_groups gives every row of the handle one int32 (n must be the handle's row count): a value >= 0 is a group id
 * (only equality matters: ids have no upper limit and need not be dense), -1 means ungrouped (never capped), any other
 * negative value is INVALID_ARG.  NULL drops the groups, a second call replaces them, a failed call leaves the previous ones.
 * Device cost: 4 B per row, a plain array in local row order; no copy of the rows is made.  Lanes share the array as they
 * share labels: a handle that has lanes refuses the call, a lane made afterwards shares the groups without a copy.
 * The _capped calls are the _diverse calls above (weights, filter and out_mmr may be NULL; a single query is k = 1) plus
 * `max_per_group` and `out_pool_rows` (may be NULL).  The pool, rel, c(i, p), mu, pen, mmr and the tie rule are those of the
 * _diverse calls bit for bit; with g_i the group of pool row i,
 *   - an unpicked pool row is ELIGIBLE at a step iff g_i == -1 or fewer than max_per_group already-picked rows have group g_i;
 *   - each step picks the eligible row with the largest mmr_i (IEEE >, a tie goes to the earlier pool position); pen is
 *     updated after every pick; the loop ends after topn picks or when no row is eligible;
 *   - *out_count = the number of picks, possibly below min(topn, P'); padding -1 / 0 / 0;
 *   - *out_pool_rows = P'.  count < topn with P' == pool: the pool ran out, raise `pool`; with P' < pool: the catalogue has
 *     no more.
 * Identities, bit for bit (ids, scores, mmr): max_per_group >= topn, or every group -1, gives the _diverse result;
 * lambda = 1.0f gives the walk of the pool in canonical order that takes a row iff it is ungrouped or fewer than
 * max_per_group earlier-taken rows share its group (the pool rows whose rank inside their group is below max_per_group, the
 * first topn of them), with out_mmr == out_score; no group id >= 0 occurs more than max_per_group times in any result; the
 * result does not depend on shard count, placement, lane or replica mode.
 * INVALID_ARG (with a message): every case of the _diverse calls; max_per_group < 1; a handle without groups.
 * mi355rec_playlist_counters counts these calls too.
 * Device: the launches of the _diverse call; mmr_rerank_kernel takes the groups and the cap as two more arguments.  In the
 * serial loop a thread counts the picks of its own group and retires at the cap; lambda == 1.0f takes a loop-free path
 * (rank in group, prefix sum over the kept rows) with the same result.
 * Node handle: one shard forwards mi355rec_sharded_set_groups and the calls; a replicated placement gives every replica the
 * whole array (a failure drops the groups on every replica); a row-sharded one keeps the host copy in the node handle and
 * passes the pool's groups to the re-rank by value, next to the pool's rows.  The CPU backend keeps a host copy and serves
 * the same calls with the same arithmetic. */
int mi355rec_set_groups(mi355rec_t* h, const int32_t* groups_host, int64_t n);
int mi355rec_sharded_set_groups(mi355rec_sharded_t* h, const int32_t* groups_host, int64_t n);
int mi355rec_query_mean_topn_capped(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                    int n_exclude, const mi355rec_filter_t* filter, float lambda, int pool, int max_per_group, int topn,
                                    int64_t* out_idx, float* out_score, float* out_mmr, int* out_count, int* out_pool_rows);
int mi355rec_query_playlist_topn_capped(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                        const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, float lambda,
                                        int pool, int max_per_group, int topn, int64_t* out_idx, float* out_score, float* out_mmr,
                                        int* out_count, int* out_pool_rows);
int mi355rec_sharded_query_mean_topn_capped(mi355rec_sharded_t* h, const float* queries, const float* weights, int k,
                                            const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                            float lambda, int pool, int max_per_group, int topn, int64_t* out_idx, float* out_score,
                                            float* out_mmr, int* out_count, int* out_pool_rows);
int mi355rec_sharded_query_playlist_topn_capped(mi355rec_sharded_t* h, const int64_t* global_rows, const float* weights, int k,
                                                const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                                float lambda, int pool, int max_per_group, int topn, int64_t* out_idx, float* out_score,
                                                float* out_mmr, int* out_count, int* out_pool_rows);

/* PLAYLIST REQUESTS: the playlist family as ONE call, and the family within LABELS ("what goes with this playlist, in rock
 * and indie, high-energy only, at most two per artist").
 * mi355rec_playlist_query_t describes one call of the family: every entry point of PLAYLISTS, FEATURE FILTERS, WEIGHTED
 * PLAYLISTS, DIVERSIFIED TOP-N and GROUP CAPS above is the special case that sets the fields it takes as arguments and leaves
 * the others zero (same checks, same launches, same results bit for bit).  The struct carries its own size as its first
 * field, as mi355rec_stats_sized does: set size = sizeof(mi355rec_playlist_query_t) of the header you compiled with.  The
 * struct only ever grows at its end; a shorter one from an older caller is read as "later fields zero"; a size of 0 (below
 * the size field itself), one that ends inside a field, or one larger than this library knows is INVALID_ARG.
 *   members / rows   exactly one is non-NULL: k x 12 floats by value, or k rows of the handle (local rows of a single handle,
 *                    global rows of a node handle; never returned);
 *   weights          NULL, or k signed weights;           exclude_global / n_exclude   as in the playlist calls;
 *   filter           NULL, or the feature filter;         topn   results asked for;
 *   labels/n_labels  NULL / 0 (every row), or the label set, see below;
 *   flags            MI355REC_PQ_DIVERSE: lambda and pool are read (the _diverse call); MI355REC_PQ_CAPPED (with _DIVERSE only):
 *                    max_per_group is read (the _capped call); MI355REC_PQ_PRIOR: prior_weight is read (ROW PRIORS below).
 *                    Unknown bits (8 and above): INVALID_ARG.
 * mi355rec_playlist_result_t: out_idx (topn slots) is required; out_score (topn), out_mmr (topn; written by diversified calls
 * only), out_count and out_pool_rows (P' of a capped call, else 0) may each be NULL.
 * THE LABEL SET.  labels[0..n_labels): values in [0, MI355REC_MAX_LABELS), duplicates allowed.  With a label set a row is
 * admissible iff its label (mi355rec_set_labels) is in the set, it passes the feature filter if there is one, and it is
 * neither excluded nor a member row.  Rows labelled -1 are never admissible; members and excluded ids need not lie in the
 * selected labels.  Everything else is unchanged bit for bit: scores, weights, canonical order, MMR picks, caps, ties.
 * count = min(topn, |admissible rows|), the rest padded with -1 / 0; a set whose labels hold no rows answers count 0 without a
 * launch; the pool of a diversified or capped call is the top-`pool` of the admissible rows.  labels == NULL with n_labels == 0
 * is exactly the call without labels (same launch, same results).  k = 1 by row with a label set returns the ids and score
 * bits of mi355rec_query_row_topn_labels.
 * INVALID_ARG (with a message): everything the family refuses; n_labels < 0; n_labels > 0 with NULL labels; labels non-NULL
 * with n_labels == 0; a label out of range; a label set on a handle without labels.
 * Device: mi355rec_set_labels also keeps the labels in row order (int16, 2 B per row); playlist_scan_kernel tests a row's
 * label against the set before anything else is done with the row (csrc/playlist.hip.h, "LABEL SET"): one pass over the
 * whole catalogue, +2 B on the 8-bit replica's 12 B per row, whatever the selection.
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one forwards the label set to
 * every shard (each holds its slice's labels from mi355rec_sharded_set_labels) and merges on the host.  The CPU backend
 * serves the same calls. */
#define MI355REC_PQ_DIVERSE 1u
#define MI355REC_PQ_CAPPED 2u
#define MI355REC_PQ_PRIOR 4u          /* ROW PRIORS below: prior_weight is read */
typedef struct {
    uint32_t size;                    /* sizeof(mi355rec_playlist_query_t) of the caller's header */
    uint32_t flags;                   /* MI355REC_PQ_* */
    const float* members;             /* k x 12 floats (host), or NULL with ... */
    const int64_t* rows;              /* ... k rows of the handle */
    const float* weights;             /* NULL, or k signed weights */
    const int64_t* exclude_global;    /* n_exclude global ids, or NULL */
    const mi355rec_filter_t* filter;  /* NULL, or the feature filter */
    const int32_t* labels;            /* NULL, or n_labels labels */
    int32_t k;
    int32_t n_exclude;
    int32_t n_labels;
    int32_t topn;
    float lambda;                     /* MI355REC_PQ_DIVERSE */
    int32_t pool;                     /* MI355REC_PQ_DIVERSE */
    int32_t max_per_group;            /* MI355REC_PQ_CAPPED */
    float prior_weight;               /* MI355REC_PQ_PRIOR (offset 84, the tail padding of older headers: sizeof stays 88) */
} mi355rec_playlist_query_t;
typedef struct {
    int64_t* out_idx;                 /* topn slots; required */
    float* out_score;                 /* topn slots, or NULL */
    float* out_mmr;                   /* topn slots, or NULL (diversified calls) */
    int* out_count;                   /* or NULL */
    int* out_pool_rows;               /* or NULL (capped calls: P') */
} mi355rec_playlist_result_t;
int mi355rec_query_playlist_request(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_playlist_result_t* result);
int mi355rec_sharded_query_playlist_request(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                            const mi355rec_playlist_result_t* result);

/* ROW PRIORS (an extension beyond the reference, which drops the dataset's `popularity` column): a per-row prior blended
 * into the ranking of the playlist request — popularity, freshness, an editorial boost, or a demotion (a negative weight:
 * "surface obscure tracks").
 * mi355rec_set_priors gives every row of the handle one fp32 (n must be the handle's row count).  Every value must be finite
 * with |p| <= 1; otherwise the call is INVALID_ARG with a message naming the first bad row.  NULL drops the priors, a second
 * call replaces them, a failed call leaves the previous ones.  Device cost: 4 B per row, a plain array in local row order,
 * padded to a whole quad of four rows (one 16-byte load serves a lane's quad).  Lanes share the array as they share groups: a
 * handle that has lanes refuses the call, a lane made afterwards shares the priors without a copy.
 * THE CALL is mi355rec_query_playlist_request with MI355REC_PQ_PRIOR set and prior_weight = beta.  The field lies at offset
 * 84, in what was the struct's tail padding (sizeof stays 88), and an older caller's padding bytes are garbage: it is read
 * ONLY when the flag is set.  With the flag set the struct's `size` must cover the field, beta must be finite with
 * |beta| <= MI355REC_MAX_PRIOR_WEIGHT, and the handle must have priors; otherwise INVALID_ARG with a message.  The twenty
 * older entry points are unchanged.
 * RANKING VALUE.  With s(x) the score the same request gives row x without the flag,
 *     v(x) = fl( s(x) + fl(beta p(x)) )         fp32, multiply then add, never fused.
 * Keys are packed from v; out_score reports v (-0.0 as +0.0); the canonical order is v descending, then row ascending; the
 * pool of a diversified or capped call is the top-`pool` by v and rel_i = v.  Admissibility (exclusion, members, filter, label
 * set), counts and padding are unchanged.
 * Identities, bit for bit: the flag with beta = 0.0f is the call without the flag (same launch, same ids and score bits); all
 * priors +0.0f is no prior; the result does not depend on shard count, placement, lane or replica mode.
 * Device: a uniform runtime branch of playlist_scan_kernel (csrc/playlist.hip.h, "ROW PRIORS"; its cut: csrc/playlist_cut.hip.h, "PRIOR"): the priors stream with the
 * 8-bit replica (+4 B on its 12 B per row) and enter the pre-filter's integer cut PER ROW; the exact chains add the prior with
 * the two operations above.  Calls without a prior take none of the new branches and never read the array.
 * Node handle: one shard forwards; a replicated placement gives every replica the whole array (a failure drops the priors on
 * every replica); a row-sharded one gives each shard its slice and merges the shards' keys on the host as before, which is
 * exact because keys carry v.  The CPU backend keeps a host copy and uses the same two operations.
 * Not served: priors on the single-query, streamed, batched and label-only routes; multiplicative blends; a separate
 * similarity output. */
#define MI355REC_MAX_PRIOR_WEIGHT 4.0f
int mi355rec_set_priors(mi355rec_t* h, const float* priors_host, int64_t n);
int mi355rec_sharded_set_priors(mi355rec_sharded_t* h, const float* priors_host, int64_t n);

/* DISTANCE REQUESTS (an extension the reference lists as "Additional Metrics: Euclidean"): the top-N rows NEAREST to up to 32
 * members by Euclidean distance over the 12 features.  Cosine ignores magnitude; on a catalogue normalised per feature (what
 * DataManager writes) the distance is a different and meaningful notion of "sounds like this".
 * The playlist request's struct is frozen, so the metric has its own struct and entry points.  mi355rec_distance_query_t carries
 * its own size under the rules of mi355rec_playlist_query_t: a shorter struct that ends where a field ends is read as "later
 * fields zero"; a size of 0, one that ends inside a field, or one larger than this library knows is INVALID_ARG.
 *   members / rows   exactly one is non-NULL: k x 12 floats by value, or k rows of the handle (local rows of a single handle,
 *                    global rows of a node handle; never returned); 1 <= k <= MI355REC_MAX_PLAYLIST;
 *   exclude_global / n_exclude, filter, labels / n_labels   as in the playlist request;
 *   topn             in [1, MI355REC_MAX_TOPN_FAST];       flags   must be 0.
 * mi355rec_distance_result_t: out_idx (topn slots) is required; out_distance (topn) and out_count may be NULL.
 * RANKING VALUE, per row x, bit for bit (fp32, subtract, multiply THEN add, never fused; members in order):
 *     d2_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fl(t * t))          (acc starts at 0.0f)
 *     m(x)    = fl( fl(...fl(d2_0 + d2_1) + ... + d2_{k-1}) / (float)k )                         (k = 1: m = d2_0)
 * Rows are ranked by m ascending, then row ascending (keys are packed from -m, so every selection and merge of the playlist
 * family serves them unchanged).  out_distance = sqrtf(m), taken on the host: for k = 1 the Euclidean distance, for k > 1 the
 * root-mean-square distance to the members — as a RANKING that is the distance to their centroid.
 * A row is admissible iff m(x) is finite (a row or member holding NaN or inf, or a sum that overflows, is never listed), it is
 * neither excluded nor a member row, it passes the feature filter if there is one and its label is in the label set if there
 * is one.  count = min(topn, |admissible rows|), the rest padded with -1 / 0.0f.
 * INVALID_ARG (with a message): flags != 0; both or neither of members and rows; a bad size; everything the playlist request
 * refuses for the fields the two share (same limits, same messages).
 * Device: a uniform runtime branch of playlist_scan_kernel (csrc/playlist.hip.h, "DISTANCE"; its cut: csrc/playlist_cut.hip.h, "DISTANCE"): no new kernel.  With the 8-bit
 * replica the scan streams 12 + 4 B per row: the replica's dot product with the members' centroid and the row's norm (a
 * 4 B/row array the handle's first distance request builds, q8_build_kernel's second output) bound m(x) from below, a per-row
 * integer cut rules rows out and only the survivors take the k chains on the fp32 rows.  The results are the same with the
 * replica on and off, bit for bit.  On a catalogue that is one tight cluster, or that has one dominant unnormalised feature,
 * the bound rules little out and the call runs at the exact path's speed.  mi355rec_playlist_counters counts these calls
 * and the rows whose chains they computed as it counts the others.
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches members given by row,
 * forwards the request to every shard and merges the shards' keys on the host, which is exact because keys carry -m.  The CPU
 * backend serves the same call with the same chain.
 * Not served: weights, diversified and capped calls, priors (there is no field for them). */
typedef struct {
    uint32_t size;                    /* sizeof(mi355rec_distance_query_t) of the caller's header */
    uint32_t flags;                   /* must be 0 */
    const float* members;             /* k x 12 floats (host), or NULL with ... */
    const int64_t* rows;              /* ... k rows of the handle */
    const int64_t* exclude_global;    /* n_exclude global ids, or NULL */
    const mi355rec_filter_t* filter;  /* NULL, or the feature filter */
    const int32_t* labels;            /* NULL, or n_labels labels */
    int32_t k;
    int32_t n_exclude;
    int32_t n_labels;
    int32_t topn;
} mi355rec_distance_query_t;
typedef struct {
    int64_t* out_idx;                 /* topn slots; required */
    float* out_distance;              /* topn slots, or NULL */
    int* out_count;                   /* or NULL */
} mi355rec_distance_result_t;
int mi355rec_query_distance_request(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_distance_result_t* result);
int mi355rec_sharded_query_distance_request(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                            const mi355rec_distance_result_t* result);

/* FEATURE SCALES: which features count, and how much.  Every ranking above compares all 12 columns at equal weight; key, mode
 * and the genre id are categorical codes on which cosine and Euclidean geometry mean little, and one dominant unnormalised
 * feature decides a distance by itself.  A scaled request takes 12 host floats a_0 .. a_11, one per column in Song.h order, beside
 * the request's struct (both structs are frozen at 88 and 64 bytes, so the scales travel in four entry points of their own).
 * DEFINITION, bit for bit: with x'_j = fl(a_j x_j) for every row and q'_kj = fl(a_j q_kj) for every member (ONE fp32 multiply
 * each), the scaled request returns exactly what the unscaled request of the same struct returns for the members q' on a
 * catalogue whose rows are x'.  The chains, member order, member weights and W, canonical order, ties, -0.0 -> +0.0, counts and
 * padding are unchanged.  Members given by row are scaled from the stored row, members given by value from the vector the caller
 * passed.  The reported score is the scaled cosine mean; out_distance is sqrtf(m') and a row is admissible for the distance
 * metric iff m' is finite.  fl(0 * NaN) is NaN and fl(0 * inf) is NaN: a zero scale does NOT hide a NaN or an inf in that column
 * (a cosine chain then answers as it does for any NaN row; a distance request never lists the row).  The feature filter tests
 * the STORED x, never x'.  Exclusion, member rows and label sets are unchanged.
 * ARGUMENTS: feature_scales == NULL is exactly the unscaled call (same launch, same results).  Otherwise every a_j is finite with
 * 0 <= a_j <= MI355REC_MAX_FEATURE_SCALE (-0.0f counts as 0), at least one a_j > 0, and the playlist struct's flags must be 0.
 * Every other check and message is the unscaled request's.  Anything else is INVALID_ARG with a message that names the feature
 * index and its value, or the refused flag.
 * IDENTITIES (tests/test_scaled_cpu.py, tests/test_gpu_scaled.py):
 *   - all scales 1.0f: the unscaled request's ids and score bits (the host routes it to the unscaled launch);
 *   - scales in {0, 1}: the request on the catalogue with those columns zeroed;
 *   - every scale times one power of two: the same cosine ids and score bits, distances times exactly that factor, as long as
 *     nothing overflows, underflows or crosses the chain's den > 1e-8 rule;
 *   - the result does not depend on shard count, placement, lane or replica mode.
 * Device: a uniform runtime branch of playlist_scan_kernel (csrc/playlist.hip.h, "FEATURE SCALES"; its cut: csrc/playlist_cut.hip.h, "SCALED"): no new kernel; calls without
 * scales take none of its branches.  A loaded row is scaled once (12 multiplies), then the unscaled chains run.  With the 8-bit
 * replica a scaled COSINE request keeps a pre-filter: the replica's dot product bounds the numerator and the row's own bytes
 * bound |Abar x^| (Abar = the scales over their maximum), a per-row integer cut rules rows out.  It is on for a_max in
 * [2^-10, 8] and members whose scaled norms are in range; rows with too little mass on the kept features take the chains.  With
 * one feature kept every cosine is +-1 and every row takes the chains.  A scaled DISTANCE request runs on the exact path (every
 * row takes the chains; the stored norms are those of the unscaled rows).
 * Measured on one MI355X at 10 M uniform rows, top-100, K = 1 (tools/run_scaled.py, profiles/r15_scaled.json): the cosine request
 * 91.4 us per call without scales, 111.9 us with key, mode and genre id at 0, 116.5 us with the scales [2,1,.5,0,1,1,3,1,.25,1,1,0];
 * K = 10: 132.9, 170.2 and 186.8 us.  The distance request 92.8 us without scales, 184.6 us scaled (212.4 us at K = 10).
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches members given by row
 * UNSCALED and forwards them by value with the scales, so each shard's fl(a_j x_j) is the by-row value; keys merge as before.
 * The CPU backend serves the same calls with the same two steps.
 * Not served: diversified and capped calls with scales; priors with scales; the re-rank's c(i,p) on scaled features; scales on
 * the single-query, streamed, batched and label-only routes; negative scales; a pre-filter for scaled distance requests. */
#define MI355REC_MAX_FEATURE_SCALE 1024.0f
int mi355rec_query_playlist_request_scaled(mi355rec_t* h, const mi355rec_playlist_query_t* query, const float* feature_scales,
                                           const mi355rec_playlist_result_t* result);
int mi355rec_query_distance_request_scaled(mi355rec_t* h, const mi355rec_distance_query_t* query, const float* feature_scales,
                                           const mi355rec_distance_result_t* result);
int mi355rec_sharded_query_playlist_request_scaled(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                   const float* feature_scales, const mi355rec_playlist_result_t* result);
int mi355rec_sharded_query_distance_request_scaled(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                   const float* feature_scales, const mi355rec_distance_result_t* result);

/* ROW SETS: exclude a listening history, or rank only within a candidate set.  exclude_global holds at most MI355REC_MAX_EXCLUDE
 * ids (they sit in LDS and are looked up after a row's chains have run); a history is 10^4 .. 10^5 tracks, and a candidate set (the
 * tracks licensed in a market, the output of a collaborative-filtering stage) is per request and arbitrary, which labels are not.
 * Both are ONE BIT PER ROW on the device: n / 8 bytes on the host and on every device copy (1.25 MB at 10 M rows).
 * A set is made once from global ids, may grow (mi355rec_rowset_add), and is passed to a request in mi355rec_request_ext_t, a
 * self-sized struct of per-request extras beside the frozen request structs: later extras extend it, not the entry points.
 * CONTRACT, bit for bit.  A row is admissible iff it was admissible without the set (not excluded, not a member row, passes the
 * filter, label in the label set, distance finite) AND (MI355REC_ROWSET_EXCLUDE: it is not in the set; MI355REC_ROWSET_ONLY: it is).
 * Everything else is the request without the set: chains, weights, priors, scales, order, ties, -0.0 -> +0.0, count = min(topn,
 * admissible rows), padding; the pool of a diversified or capped call is the top-`pool` of the admissible rows.  Members may lie
 * inside or outside the set and are never returned.  A set goes with every flag of the playlist request; with feature_scales the
 * playlist flags must be 0, as for the _scaled call.
 * IDENTITIES (tests/test_rowset_cpu.py, tests/test_gpu_rowset.py):
 *   - ext == NULL, or both of its pointers NULL: the plain request (same launch, same ids and bits); scales only: the _scaled call;
 *   - EXCLUDE with |S| <= MI355REC_MAX_EXCLUDE: the request with S appended to exclude_global; EXCLUDE with an empty set (and ONLY
 *     with every row): the plain request, launched as such;
 *   - ONLY with an empty set, EXCLUDE with every row: count 0, nothing is launched;
 *   - the result does not depend on replica mode, lane, shard count or placement.
 * IDS: duplicates allowed, any order.  Single handle: 0 <= id < 2^32 as for exclude_global, ids outside [row_base, row_base + n)
 * match nothing.  Node handle: 0 <= id < n.  A negative or too large id (named in the message), n_ids < 0, or a NULL list with
 * n_ids > 0 is INVALID_ARG; n_ids == 0 makes an empty set.  A failed mi355rec_rowset_add leaves the set unchanged.  Errors of create
 * are the handle's last error, those of add are mi355rec_last_global_error().
 * OWNERSHIP: a set belongs to the handle it was made on and may be used on it and on its lanes (same rows, same device); a node
 * handle's set on that node handle only; anything else is INVALID_ARG ("row set of another handle").  Sets are destroyed BEFORE
 * their handle.  Requests only read a set, so requests on different lanes may share one at the same time; mi355rec_rowset_add or
 * _destroy concurrent with a request that uses the set is the caller's error.
 * mi355rec_rowset_count: the distinct rows of the handle in the set.  create and add copy to the device synchronously before they
 * return; add uploads the whole bitmap of every copy again.
 * Device (csrc/playlist.hip.h, "ROW SETS"): no new kernel and no second instantiation: a uniform branch of playlist_scan_kernel.
 * Per tile a lane reads its quad's four bits and clears the rows the set rejects BEFORE the label test, the 8-bit dot products, the
 * filter's fp32 loads and any chain, on the exact path too: a rejected row costs one bit and mi355rec_playlist_counters' rows_exact
 * does not count it.  A request without a set reads nothing new.  A row-sharded node gives every shard its slice of the bitmap, a
 * replicated one every replica the whole; the CPU backend tests the host bitmap.  The call always makes one pass over the catalogue.
 * Measured on one MI355X at 10 M uniform rows, top-100, replica on, K = 1 by row (tools/run_rowset.py, profiles/r17_rowset.json; p50
 * per call): the cosine request 92.2 us without a set, 100.4 us with a set that rejects nothing returnable, 100.5 us with 20 000
 * random ids excluded, 101.2 us within a random half, 83.9 us within a random 1 %; K = 10: 134.6, 142.5, 142.5, 138.4, 118.8 us; the
 * distance request, K = 1: 94.8, 98.2, 98.1, 96.7, 81.5 us.  Calls without a set are within the parent build's own spread
 * (profiles/r17_rowset_ab.json).
 * Not served: sets on the single-query, streamed, batched and label-only routes; two sets in one request; removing ids; set
 * algebra.  (A request that names its candidates reads only those rows: CANDIDATE LISTS below.) */
typedef struct mi355rec_rowset mi355rec_rowset_t;
int mi355rec_rowset_create(mi355rec_t* h, const int64_t* global_ids, int64_t n_ids, mi355rec_rowset_t** out);
int mi355rec_sharded_rowset_create(mi355rec_sharded_t* h, const int64_t* global_ids, int64_t n_ids, mi355rec_rowset_t** out);
int mi355rec_rowset_add(mi355rec_rowset_t* s, const int64_t* global_ids, int64_t n_ids);
int64_t mi355rec_rowset_count(const mi355rec_rowset_t* s);
void mi355rec_rowset_destroy(mi355rec_rowset_t* s);   /* NULL is fine */

#define MI355REC_ROWSET_EXCLUDE 0u   /* rows IN the set are not admissible ("seen") */
#define MI355REC_ROWSET_ONLY 1u      /* rows NOT in the set are not admissible ("candidates") */
typedef struct {
    uint32_t size;                     /* sizeof of the caller's header; the size rules of mi355rec_playlist_query_t */
    uint32_t rowset_mode;              /* MI355REC_ROWSET_*; read only where rowset != NULL; other values INVALID_ARG */
    const float* feature_scales;       /* NULL, or 12 scales: exactly the _scaled call's argument */
    const mi355rec_rowset_t* rowset;   /* NULL, or the set */
} mi355rec_request_ext_t;              /* 24 bytes */
int mi355rec_query_playlist_request_ext(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_request_ext_t* ext,
                                        const mi355rec_playlist_result_t* result);
int mi355rec_query_distance_request_ext(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_request_ext_t* ext,
                                        const mi355rec_distance_result_t* result);
int mi355rec_sharded_query_playlist_request_ext(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                const mi355rec_request_ext_t* ext, const mi355rec_playlist_result_t* result);
int mi355rec_sharded_query_distance_request_ext(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                const mi355rec_request_ext_t* ext, const mi355rec_distance_result_t* result);

/* CANDIDATE LISTS: "rank these few thousand candidates", the second stage of a two-stage recommender (the first stage being
 * collaborative filtering, a market's licensed tracks, a search hit list).  An ONLY row set serves it with n / 8 bytes of bitmap built
 * and uploaded per request and one pass over the whole catalogue.  A request may instead carry the LIST itself: n_candidates global
 * row ids, any order, duplicates allowed.  Only listed rows are admissible; the engine GATHERS exactly those rows, scores them with
 * the request's own exact chain and selects the top-N.  The list is an argument of four entry points (mi355rec_request_ext_t keeps
 * its 24 bytes), which otherwise are the _ext calls: ext may be NULL.
 * CONTRACT, bit for bit.  A request with the list C returns what the same request returns with an ONLY row set made from C and no
 * list: ids, order, score bits, out_count, out_mmr, out_pool_rows, padding.  Everything else keeps its meaning and its arithmetic:
 * exclusion list, member rows, filter, label set, prior, weights, MMR, caps, distance, scales.  If ext carries a row set S as well,
 * both must admit a row: ONLY S ranks within C n S, EXCLUDE S within C \ S (candidates minus a listening history, the common
 * pairing).  Members may be listed and are never returned.  The result does not depend on replica mode, lane, shard count or
 * placement.
 * ARGUMENTS: every check and message of the _ext call comes first, then the list's: n_candidates == 0 is an empty list (count 0,
 * padded, nothing is launched); a NULL list with n_candidates > 0, n_candidates < 0 and n_candidates > MI355REC_MAX_CANDIDATES
 * (4 MB of staged ids) are INVALID_ARG.  Single handle: an id below 0 or at or above 2^32 is INVALID_ARG (named in the message, as
 * for row sets); ids outside [row_base, row_base + n) match nothing.  Node handle: an id below 0 or at or above n is INVALID_ARG.
 * HOST (csrc/candidates.h): the list is reduced to the shard's sorted, distinct local rows as uint32 (one pass checks the ids on a
 * single handle, keeps those of the shard and tests whether they already ascend strictly: then nothing is sorted), staged through a pinned buffer of the handle and copied on the
 * handle's stream ahead of the launch; both buffers grow on demand.  A row-sharded node gives each shard the ids of its range (a
 * shard with none launches nothing), a replicated one gives the serving replica the whole list, the CPU backend searches the
 * sorted list per row.
 * DEVICE (csrc/playlist.hip.h, "CANDIDATE LISTS"): no new kernel and no second instantiation: a uniform branch of
 * playlist_scan_kernel in place of the anchor bound and the tile scan.  A thread takes two consecutive entries and requests their
 * rows together (kPlGatherPerThread: a tuning constant of the kernel, no part of this interface); the launch has one workgroup of 512
 * threads per 1024 rows, up to the handle's grid.  The replica
 * is never consulted: every listed row that passes the row set and the label test takes the exact chain and counts into
 * mi355rec_playlist_counters' rows_exact.  A request without a list takes the path it took before.
 * mi355rec_candidates_counters: requests = requests that took the gather launch (an empty shard list launches nothing and is not
 * counted); rows_gathered = the distinct in-shard list entries those launches were given.  Either pointer may be NULL.
 * Measured on one MI355X at 10 M uniform rows, top-100, replica on, K = 1 by row (tools/run_candidates.py,
 * profiles/r19_candidates.json; p50 per call), the list ascending: 38.2 us at 100 ids, 42.3 at 1 000, 66.5 at 10 000, 139.4 at 100
 * 000, 796 at 1 000 000, beside 68.3 / 71.7 / 77.0 / 84.6 / 106.7 us with a pre-made ONLY set of the same ids, 299 ... 1 498 us with
 * an ONLY set made per request and 92.0 us without list or set; a shuffled list adds the host's sort: 3 us at 1 000 ids, 316 us at
 * 10 000, 4.1 ms at 100 000, 48 ms at 1 000 000.  The gather stops winning over the pre-made ONLY set between 10 000 and 100 000 ids
 * for an ascending list and between 1 000 and 10 000 for a shuffled one (K = 10 and the distance request alike).
 * MI355REC_MAX_CANDIDATES bounds the staging buffer; it is no routing threshold.  A thread takes two entries, not four, because the
 * kernel sits on its register budget: 4 entries per thread need scratch (docs/LAB_NOTES.md).  Requests without a list are within the
 * parent build's own spread (profiles/r19_candidates_ab.json).
 * Not served: routing a small ONLY row set to the gather by itself; lists on the single-query, streamed, batched and label-only
 * routes; a pre-filter for the gather (every listed row takes the exact chain).  (Scores of candidates outside the top-N:
 * CANDIDATE SCORES below.) */
#define MI355REC_MAX_CANDIDATES 1048576
int mi355rec_query_playlist_request_candidates(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, const mi355rec_playlist_result_t* result);
int mi355rec_query_distance_request_candidates(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, const mi355rec_distance_result_t* result);
int mi355rec_sharded_query_playlist_request_candidates(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       const mi355rec_playlist_result_t* result);
int mi355rec_sharded_query_distance_request_candidates(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       const mi355rec_distance_result_t* result);
int mi355rec_candidates_counters(const mi355rec_t* h, int64_t* requests, int64_t* rows_gathered);

/* CANDIDATE SCORES: "how does this request value these candidates", for a blender or re-ranker that mixes the first stage's own
 * score with the engine's and so needs the value of EVERY candidate, not of the N best.  The calls take what the _candidates calls
 * take, with two arrays of n_candidates entries in place of the result struct.
 * CONTRACT, bit for bit, for every i in [0, n_candidates), g = candidates[i]: g is ADMISSIBLE iff the matching _candidates call
 * with the same query and ext and the one-entry list {g} returns g.  Then out_value[i] holds the bits of that call's out_score[0]
 * (out_distance[0] = sqrtf(m) for the distance call) and out_admissible[i] is 1.  Otherwise out_value[i] is the quiet NaN
 * 0x7fc00000 and out_admissible[i] is 0: an excluded id, a member given by row, a row that the row set, the label set or the
 * filter rejects, a distance that is not finite and, on a single handle, an id outside [row_base, row_base + n).  Output is in
 * list order; duplicates each get their value; a score of -0.0 reports as +0.0; weights, MI355REC_PQ_PRIOR (the value is v),
 * feature scales and both row-set modes keep their meaning.  The result does not depend on replica mode, lane, shard count or
 * placement.
 * ARGUMENTS: every check and message of the _candidates call first (topn included: one struct serves both calls; topn is otherwise
 * unused).  Then: MI355REC_PQ_DIVERSE and MI355REC_PQ_CAPPED are INVALID_ARG (a re-ranked order has no per-row value); a NULL
 * out_value with n_candidates > 0 is INVALID_ARG; out_admissible may be NULL.  n_candidates == 0 returns OK, writes nothing and
 * launches nothing.
 * DEVICE (csrc/playlist.hip.h, "CANDIDATE SCORES"): no new kernel: the gather launch with topk == 0 stores the key of entry e of
 * the shard's sorted, distinct list (or 0) at index e of a per-handle buffer of 8 B per entry, which grows on demand, and selects
 * nothing; no merge is launched.  The host copies the buffer back through a pinned one on the handle's stream and unpacks it
 * through the list-order map of csrc/candidates.h.  A scoring launch is a gather launch: it counts into
 * mi355rec_candidates_counters and rows_exact as the _candidates call with the same list does.
 * Measured on one MI355X at 10 M uniform rows, K = 1 by row, replica on, the list ascending (tools/run_candidate_scores.py,
 * profiles/r21_candidate_scores.json; p50 per call beside the _candidates top-100 call on the same list): 32.9 us against 40.2 at
 * 100 ids, 35.9 / 43.8 at 1 000, 84.3 / 67.2 at 10 000, 281.8 / 140.3 at 100 000, 2 225 / 800 at 1 000 000: faster while the saved
 * merge launch shows, slower from 10 000 ids, where the host's work per id (the list-order map, the copy back, the unpack) outgrows
 * it.  Requests without a list and _candidates requests are within the parent build's own spread (profiles/r21_candidate_scores_ab.json).
 * Not served: scores on the single-query, streamed, batched and label-only routes; per-member scores; asynchronous variants. */
int mi355rec_score_playlist_request_candidates(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, float* out_value,
                                               uint8_t* out_admissible /* may be NULL */);
int mi355rec_score_distance_request_candidates(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, float* out_distance,
                                               uint8_t* out_admissible /* may be NULL */);
int mi355rec_sharded_score_playlist_request_candidates(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       float* out_value, uint8_t* out_admissible /* may be NULL */);
int mi355rec_sharded_score_distance_request_candidates(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       float* out_distance, uint8_t* out_admissible /* may be NULL */);

/* ANY-OF REQUESTS ("multi-interest" retrieval): the top-N rows by their BEST match among up to 32 members ("like any of these"),
 * and which member each result matched ("because you listened to X").  The mean and the distance requests collapse a playlist
 * to one point (its mean direction, its centroid); a listener with two tastes gets the songs in between.  This request does not.
 * mi355rec_anyof_query_t carries its own size under the rules of mi355rec_playlist_query_t.
 *   members / rows   exactly one is non-NULL: k x 12 floats by value, or k rows of the handle (local rows of a single handle,
 *                    global rows of a node handle; never returned); 1 <= k <= MI355REC_MAX_PLAYLIST;
 *   exclude_global / n_exclude, filter, labels / n_labels   as in the playlist request;
 *   topn             in [1, MI355REC_MAX_TOPN_FAST];       flags   must be 0.
 * mi355rec_anyof_result_t: out_idx (topn slots) is required; out_score, out_member (topn slots each) and out_count may be NULL.
 * RANKING VALUE, per row x, bit for bit:
 *     c_k(x) = the score mi355rec_query_topn gives row x for the query q_k        (never NaN, in [-1, 1])
 *     v(x) = c_0;  a(x) = 0;   for k = 1 .. K-1:  if (c_k > v) { v = c_k; a = k; }   (IEEE compare: -0.0 does not beat +0.0)
 * Rows rank by v descending, then row ascending (keys are packed from v: -0.0 reports as +0.0).  out_score[i] = v and
 * out_member[i] = a of result i: the SMALLEST index into the caller's member list that attains the maximum.
 * count = min(topn, |admissible rows|); past it the padding is -1 / +0.0f / -1.  Admissibility is the playlist request's (not
 * excluded, not a member row, the filter, the label set, the row set of `ext`).
 * ext: may be NULL; its row set is honoured with the _ext calls' ownership checks; a non-NULL feature_scales is INVALID_ARG
 * ("any-of requests take no feature scales").  There are no _ext or _scaled variants: this one entry point takes ext.
 * INVALID_ARG (with a message): flags != 0; both or neither of members and rows; a bad size; everything the playlist request
 * refuses for the fields the two share (same limits, same messages).
 * Device: anyof_scan_kernel (csrc/anyof.hip.h), the playlist scan's launch geometry.  With the 8-bit replica the row a lane holds
 * is dotted with every member (6 v_dot4_i32_i8 per member and row) and a row is ruled out only if EVERY member's cut rules it out
 * (csrc/playlist_cut.hip.h, "ANY"); the survivors take the k chains on the fp32 row.  Replica on and off answer alike, bit for
 * bit.  out_member costs a second, tiny launch of the same kernel over the merged result rows.  mi355rec_playlist_counters counts
 * these calls and the rows whose chains they computed (the attribution's rows not included).
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches members given by row,
 * forwards them by value to every shard and merges keys and member indices on the host.  The CPU backend serves the same call.
 * Measured (MI355X, 10 M uniform rows, top-100, 8-bit replica on; profiles/r22_anyof.json), p50 per call in us,
 * any-of / any-of with out_member / K one-member playlist requests + host merge / mean playlist request:
 *     K = 1: 86.1 / 102.1 / 106.2 / 93.7      K = 3: 101.8 / 116.4 / 322.2 / 100.9
 *     K = 10: 180.5 / 196.8 / 1094.5 / 133.9   K = 32: 435.3 / 456.2 / 3689.3 / 242.8
 * The request beats the K one-member requests at every K measured; 4 - 6 % of the rows take the chains, as for the mean request
 * (has the 300-cluster sorted catalogue as well).
 * Not served: weights, priors, feature scales, MMR and caps; an any-of distance; candidate lists and scores; asynchronous,
 * streamed or batched variants. */
typedef struct {
    uint32_t size;                    /* sizeof(mi355rec_anyof_query_t) of the caller's header */
    uint32_t flags;                   /* must be 0 */
    const float* members;             /* k x 12 floats (host), or NULL with ... */
    const int64_t* rows;              /* ... k rows of the handle */
    const int64_t* exclude_global;    /* n_exclude global ids, or NULL */
    const mi355rec_filter_t* filter;  /* NULL, or the feature filter */
    const int32_t* labels;            /* NULL, or n_labels labels */
    int32_t k;
    int32_t n_exclude;
    int32_t n_labels;
    int32_t topn;
} mi355rec_anyof_query_t;             /* 64 bytes */
typedef struct {
    int64_t* out_idx;                 /* topn slots; required */
    float* out_score;                 /* topn slots, or NULL */
    int32_t* out_member;              /* topn slots, or NULL */
    int* out_count;                   /* or NULL */
} mi355rec_anyof_result_t;
int mi355rec_query_anyof_request(mi355rec_t* h, const mi355rec_anyof_query_t* query, const mi355rec_request_ext_t* ext,
                                 const mi355rec_anyof_result_t* result);
int mi355rec_sharded_query_anyof_request(mi355rec_sharded_t* h, const mi355rec_anyof_query_t* query, const mi355rec_request_ext_t* ext,
                                         const mi355rec_anyof_result_t* result);

/* MANHATTAN REQUESTS (the reference lists "Additional Metrics: Euclidean, Manhattan distance" among its extensions): the top-N
 * rows NEAREST by L1 distance to up to 32 members.  Where the distance request squares a coordinate's difference, this one does
 * not: one badly-off feature does not dominate.  mi355rec_manhattan_query_t has the field list of mi355rec_distance_query_t and
 * carries its own size under the same rules.
 *   members / rows   exactly one is non-NULL: k x 12 floats by value, or k rows of the handle (never returned);
 *                    1 <= k <= MI355REC_MAX_PLAYLIST;
 *   exclude_global / n_exclude, filter, labels / n_labels   as in the playlist request;
 *   topn             in [1, MI355REC_MAX_TOPN_FAST];       flags   must be 0.
 * mi355rec_manhattan_result_t: out_idx (topn slots) is required; out_distance (topn slots) and out_count may be NULL.
 * RANKING VALUE, per row x, bit for bit in fp32, never fused:
 *     d1_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fabsf(t))              (acc starts at 0.0f)
 *     m(x)    = fl( fl(...fl(d1_0 + d1_1) + ... + d1_{K-1}) / (float)K )                            (members in order)
 * Rows rank by m ascending, then row ascending.  Keys are packed from -m as the distance request's are (m = 0 packs as +0.0);
 * out_distance[i] = m itself (0.0f - score: no root).  A row whose m is not finite forms no key.  Admissibility is the playlist
 * request's (the row set of `ext`, the label set, the filter, not a member row, not excluded); count = min(topn, |admissible
 * rows|), past it the padding is -1 / +0.0f.
 * ext: may be NULL; its row set is honoured with the _ext calls' ownership checks; a non-NULL feature_scales is INVALID_ARG
 * ("manhattan requests take no feature scales").  There are no _ext or _scaled variants: this one entry point takes ext.
 * INVALID_ARG (with a message): flags != 0; both or neither of members and rows; a bad size; everything the playlist request
 * refuses for the fields the two share (same limits, same messages).
 * Device: manhattan_scan_kernel (csrc/anyof.hip.h, "MANHATTAN": any-of's pieces instantiated for this metric in a kernel of their
 * own): the playlist scan's launch, the members in LDS.
 * With the 8-bit replica and the handle's per-row norms (the distance request's: built on first use, dropped by
 * mi355rec_rebuild_replica, kept exact by mi355rec_update_rows) a row costs 16 B: its bytes times its stored norm give a point
 * within half a replica step per coordinate of the row, and the PER-MEMBER sum of L1 distances to that point, less 12 half steps,
 * bounds m from below; a row whose bound exceeds the workgroup's threshold is ruled out, the others take the chains on the fp32
 * row.  Replica on and off answer alike, bit for bit.  mi355rec_playlist_counters counts these calls and their rows_exact.
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches members given by row,
 * forwards them by value to every shard and merges keys of -m on the host.  The CPU backend runs the same chain.
 * Measured (MI355X, 10 M uniform rows, top-100, members by row; profiles/r23_manhattan.json, tools/run_manhattan.py), p50 per call
 * in us, on a handle with the replica / on one without, and the distance and any-of requests with the replica beside it:
 *     K = 1: 97.2 / 192.5, 97.8, 89.6      K = 3: 113.8 / 195.3, 100.1, 103.8
 *     K = 10: 184.2 / 212.3, 119.0, 184.0   K = 32: 280.0 / 270.9, 187.7, 434.4
 * The bound's arithmetic grows with K as the chains' does.  With the bound at every K (profiles/r23_manhattan_cut_every_k.json) it
 * wins at K = 1, 3, 10 (97.7 / 113.6 / 185.4 us) and loses at K = 32 (416.1 us against 270.9 without a replica), so it is used up
 * to K = 10: ABOVE THAT THE LAUNCH IS THE EXACT PATH WHATEVER THE HANDLE HOLDS (the K = 32 figure "with the replica" above is the
 * chains on every row).  3.5 - 4.3 % of the rows take the chains up to K = 10.  Against the parent commit's library
 * (profiles/r23_manhattan_ab.json) the any-of, playlist and distance requests did not move (five alternating
 * children a side: no ratio above 1, each inside the parent's own spread).
 * Not served: weights, priors, feature scales, MMR and caps; candidate lists and candidate scores; asynchronous, streamed and
 * batched variants; the torch.distributed ShardedEngine; a cheaper cut for large K (per coordinate mean_k |q_kj - t| is convex
 * and piecewise linear in t: an evaluation that does not touch all K members is the next step). */
typedef struct {
    uint32_t size;                    /* sizeof(mi355rec_manhattan_query_t) of the caller's header */
    uint32_t flags;                   /* must be 0 */
    const float* members;             /* k x 12 floats (host), or NULL with ... */
    const int64_t* rows;              /* ... k rows of the handle */
    const int64_t* exclude_global;    /* n_exclude global ids, or NULL */
    const mi355rec_filter_t* filter;  /* NULL, or the feature filter */
    const int32_t* labels;            /* NULL, or n_labels labels */
    int32_t k;
    int32_t n_exclude;
    int32_t n_labels;
    int32_t topn;
} mi355rec_manhattan_query_t;         /* 64 bytes */
typedef struct {
    int64_t* out_idx;                 /* topn slots; required */
    float* out_distance;              /* topn slots, or NULL: m(x) */
    int* out_count;                   /* or NULL */
} mi355rec_manhattan_result_t;
int mi355rec_query_manhattan_request(mi355rec_t* h, const mi355rec_manhattan_query_t* query, const mi355rec_request_ext_t* ext,
                                     const mi355rec_manhattan_result_t* result);
int mi355rec_sharded_query_manhattan_request(mi355rec_sharded_t* h, const mi355rec_manhattan_query_t* query,
                                             const mi355rec_request_ext_t* ext, const mi355rec_manhattan_result_t* result);

/* BOUNDED REQUESTS: "only rows that are good enough" and "how many such rows are there".  Every other request answers "which N
 * rows are best"; topn is capped at MI355REC_MAX_TOPN_FAST, so a caller that cuts a returned list at a score cannot learn how many
 * rows pass.  A bounded request takes a BOUND beside the fields of the distance request: a score floor for the cosine metric, a
 * radius for the Euclidean one.  It returns the leading matching rows and the EXACT number of matching rows, whatever topn is.
 * mi355rec_bounded_query_t has the field list of mi355rec_distance_query_t followed by `metric` and `bound`, and carries its own
 * size under the same rules (every field end is a valid size; a shorter struct reads as "later fields zero").
 *   members / rows   exactly one is non-NULL: k x 12 floats by value, or k rows of the handle (never returned, never counted);
 *                    1 <= k <= MI355REC_MAX_PLAYLIST;
 *   exclude_global / n_exclude, filter, labels / n_labels   as in the playlist request;
 *   topn             in [0, MI355REC_MAX_TOPN_FAST]; 0: count only;       flags   must be 0;
 *   metric           MI355REC_BOUNDED_COSINE or MI355REC_BOUNDED_EUCLIDEAN;
 *   bound            cosine: the floor, any finite value; Euclidean: the radius, finite and >= 0.
 * mi355rec_bounded_result_t: out_total is required; out_idx and out_score (topn slots each) may be NULL when topn == 0 (out_idx is
 * required otherwise, out_score may always be NULL); out_count may be NULL.
 * Admissibility is the playlist request's, unchanged: the row set of `ext`, the label set, the filter, not a member row, not excluded.
 * RANKING VALUE AND KEY, per metric:
 *   MI355REC_BOUNDED_COSINE     the playlist request's unweighted mean cosine: bit for bit the score mi355rec_query_playlist_request
 *                               reports with flags 0;
 *   MI355REC_BOUNDED_EUCLIDEAN  the distance request's m(x) ("DISTANCE REQUESTS"), keys of -m; the reported value is sqrtf(m).
 * A row MATCHES iff it is admissible and its key exceeds floor_thr = (uint64(ordered image of b) << 32) - 1, the ordered image
 * being the one keys carry (mi355rec_key_score's inverse; -0.0 and +0.0 share one):
 *   cosine      b = bound: score >= bound.  Above 1 nothing matches; at -1 or below every admissible row does;
 *   Euclidean   b = -m_max, m_max the largest float with sqrtf(m_max) <= bound (found on the host from fl(bound^2) by nextafterf
 *               steps: sqrtf is monotone): a row matches exactly when the distance the call would report is <= the radius.  A
 *               row whose m is not finite never matches.
 * OUTPUT: *out_total = the number of matching rows, exact; count = min(topn, total); results [0, count) are the matching rows in
 * key order: exactly the leading matching results of the unbounded playlist or distance request with the same fields (ids, order,
 * score bits); past count the padding is -1 / +0.0f.
 * INVALID_ARG (with a message): a NaN or infinite bound; a negative radius; an unknown metric; flags != 0; topn out of range; a
 * non-NULL feature_scales in ext ("bounded requests take no feature scales"); both or neither of members and rows; a bad size;
 * everything the playlist request refuses for the fields the two share (same limits, same messages).
 * Device: no new kernel.  At most two launches of playlist_scan_kernel on the handle's stream: the COUNT launch, always (the scan
 * with topk == 0: csrc/playlist.hip.h, "BOUNDED"), then, for topn > 0, the ordinary top-N launch of the same request and its
 * merge; the host cuts the merged results at the floor.  The count launch starts at the floor, so the 8-bit pre-filter runs at
 * its final cut from the first tile; a row the cut leaves takes the exact chains, and key > floor_thr then the exclusion lookup
 * decide.  With the cosine metric and no feature filter the replica also proves rows IN (csrc/playlist_cut.hip.h, "BOUNDED": the
 * bound is symmetric): such a row is counted without its fp32 row being read, and only the band between the two cuts takes the
 * chains.  Replica on and off answer alike, bit for bit.  mi355rec_playlist_counters counts the call ONCE; its rows_exact moves
 * for the top-N launch only, NOT for count launches (their counter word is the call's total).
 * Measured (MI355X, 10 M uniform rows, K = 1 by row, p50 per call; profiles/r26_bounded.json, tools/run_bounded.py; the parent
 * commit's plain top-100 playlist request: 95.4 us): count only at a floor about 1 000 rows pass 60.5 us; count only at the median
 * floor (5.0 M matches) 95.3 us (152.2 us with the proven-in shortcut off: profiles/r26_bounded_shortcut_ab.json); topn = 100 with
 * the tight floor 110.6 us, with the median floor 169.4 us.  The existing requests against the parent's library
 * (profiles/r26_bounded_existing_ab.json): ratios 0.995 - 1.013, all but distance K = 10 (1.013 against 1.2 %) inside its spread.
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches members given by row,
 * forwards them by value to every shard, merges keys on the host, cuts at the floor and sums the shards' totals.  The CPU
 * backend runs the same chain, floor and total.
 * Not served (refused or absent): weights, diversified and capped calls, priors, feature scales, candidate lists, the any-of and
 * Manhattan metrics; asynchronous, streamed and batched variants. */
#define MI355REC_BOUNDED_COSINE 0
#define MI355REC_BOUNDED_EUCLIDEAN 1
typedef struct {
    uint32_t size;                    /* sizeof(mi355rec_bounded_query_t) of the caller's header */
    uint32_t flags;                   /* must be 0 */
    const float* members;             /* k x 12 floats (host), or NULL with ... */
    const int64_t* rows;              /* ... k rows of the handle */
    const int64_t* exclude_global;    /* n_exclude global ids, or NULL */
    const mi355rec_filter_t* filter;  /* NULL, or the feature filter */
    const int32_t* labels;            /* NULL, or n_labels labels */
    int32_t k;
    int32_t n_exclude;
    int32_t n_labels;
    int32_t topn;                     /* 0: count only */
    int32_t metric;                   /* MI355REC_BOUNDED_COSINE, MI355REC_BOUNDED_EUCLIDEAN */
    float bound;                      /* the score floor, or the radius */
} mi355rec_bounded_query_t;           /* 72 bytes */
typedef struct {
    int64_t* out_idx;                 /* topn slots; may be NULL when topn == 0 */
    float* out_score;                 /* topn slots, or NULL: the score, or (Euclidean) the distance */
    int* out_count;                   /* or NULL: min(topn, total) */
    int64_t* out_total;               /* required: the number of matching rows */
} mi355rec_bounded_result_t;
int mi355rec_query_bounded_request(mi355rec_t* h, const mi355rec_bounded_query_t* query, const mi355rec_request_ext_t* ext,
                                   const mi355rec_bounded_result_t* result);
int mi355rec_sharded_query_bounded_request(mi355rec_sharded_t* h, const mi355rec_bounded_query_t* query,
                                           const mi355rec_request_ext_t* ext, const mi355rec_bounded_result_t* result);

/* JACCARD REQUESTS (the reference's README names "additional similarity metrics (Euclidean, Jaccard)" among its extensions): the
 * top-N rows by WEIGHTED JACCARD (Ruzicka) similarity to up to 32 members.  Unlike cosine it sees how large the features are, not
 * only their direction.  mi355rec_jaccard_query_t has the field list of mi355rec_distance_query_t and carries its own size under
 * the same rules.
 *   members / rows   exactly one is non-NULL: k x 12 floats by value, or k rows of the handle (never returned);
 *                    1 <= k <= MI355REC_MAX_PLAYLIST;
 *   exclude_global / n_exclude, filter, labels / n_labels   as in the playlist request;
 *   topn             in [1, MI355REC_MAX_TOPN_FAST];       flags   must be 0.
 * mi355rec_jaccard_result_t: out_idx (topn slots) is required; out_similarity (topn slots) and out_count may be NULL.
 * RANKING VALUE, per member k and row x, bit for bit in fp32, in this order, never fused:
 *     num = den = 0.0f
 *     for j = 0..11:  lt = x_j < q_kj;  lo = lt ? x_j : q_kj;  hi = lt ? q_kj : x_j;
 *                     num = fl(num + lo);  den = fl(den + hi)
 *     J_k  = fl(num / den)                                                             (one IEEE divide)
 *     v(x) = fl( fl(...fl(J_0 + J_1) + ... + J_{K-1}) / (float)K )                     (members in order; K = 1 divides by 1.0f)
 * min and max are ONE compare and two selects, not fminf / fmaxf (which drop a NaN): a NaN in the row reaches den, a NaN in a
 * member reaches num.  Rows rank by v descending, then row ascending (keys are pack_key(v, global row));
 * out_similarity[i] = v.  A row forms a key only if v is finite and every den_k is below +inf (a +inf feature would otherwise
 * score a quiet 0): two all-zero vectors (0 / 0), NaN and infinite features are never returned, and the count says so.  The
 * formula is applied as written whatever the signs; it is the Ruzicka similarity, in [0, 1], where row and members are
 * non-negative, which a min-max normalised catalogue always is.  A copy of the single member scores exactly 1.0f.
 * Admissibility is the playlist request's (the row set of `ext`, the label set, the filter, not a member row, not excluded);
 * count = min(topn, |admissible rows that form a key|), past it the padding is -1 / +0.0f.
 * ext: may be NULL; its row set is honoured with the _ext calls' ownership checks; a non-NULL feature_scales is INVALID_ARG
 * ("jaccard requests take no feature scales").  There are no _ext or _scaled variants: this one entry point takes ext.
 * INVALID_ARG (with a message): flags != 0; both or neither of members and rows; a bad size; everything the playlist request
 * refuses for the fields the two share (same limits, same messages).
 * Device: no new kernel.  playlist_scan_kernel (csrc/playlist.hip.h, "JACCARD") takes a third value of PlaylistArg::metric, a
 * uniform branch of playlist_row_key: the K chains above in place of the cosine chains.  The kernel stays at 128 VGPRs, 40 128 B
 * of LDS and no scratch; the library holds 60 kernels.
 * NO PRE-FILTER: every row takes the chains, on a handle with the 8-bit replica as on one without (the launch is given no
 * replica).  An 8-bit bound is proven (docs/LAB_NOTES.md) but the forms tried reserve scratch in a kernel that sits on its
 * register budget, which the build refuses.  mi355rec_playlist_counters counts these calls; rows_exact grows by every row read.
 * Node handle: one shard forwards; a replicated placement asks one replica; a row-sharded one fetches members given by row,
 * forwards them by value to every shard and merges keys of v on the host.  The CPU backend runs the same chain.
 * Measured (MI355X, 10 M uniform rows, top-100, members by row; profiles/r27_jaccard.json, tools/run_jaccard.py), p50 per call in
 * us, on a handle with the replica / on one without (the same launch):
 *     K = 1: 189.2 / 188.2      K = 3: 206.4 / 205.0      K = 10: 268.2 / 264.1      K = 32: 572.9 / 574.2
 * (the cosine, distance and Manhattan requests on the handle without a replica, every row exact: 187.9, 184.2, 193.1 at K = 1 and
 * 432.1, 338.6, 275.6 at K = 32).
 * Not served: weights, priors, feature scales, MMR and caps; bounds; candidate lists and candidate scores; asynchronous,
 * streamed and batched variants; the torch.distributed ShardedEngine. */
typedef struct {
    uint32_t size;                    /* sizeof(mi355rec_jaccard_query_t) of the caller's header */
    uint32_t flags;                   /* must be 0 */
    const float* members;             /* k x 12 floats (host), or NULL with ... */
    const int64_t* rows;              /* ... k rows of the handle */
    const int64_t* exclude_global;    /* n_exclude global ids, or NULL */
    const mi355rec_filter_t* filter;  /* NULL, or the feature filter */
    const int32_t* labels;            /* NULL, or n_labels labels */
    int32_t k;
    int32_t n_exclude;
    int32_t n_labels;
    int32_t topn;
} mi355rec_jaccard_query_t;           /* 64 bytes */
typedef struct {
    int64_t* out_idx;                 /* topn slots; required */
    float* out_similarity;            /* topn slots, or NULL: v(x) */
    int* out_count;                   /* or NULL */
} mi355rec_jaccard_result_t;
int mi355rec_query_jaccard_request(mi355rec_t* h, const mi355rec_jaccard_query_t* query, const mi355rec_request_ext_t* ext,
                                   const mi355rec_jaccard_result_t* result);
int mi355rec_sharded_query_jaccard_request(mi355rec_sharded_t* h, const mi355rec_jaccard_query_t* query,
                                           const mi355rec_request_ext_t* ext, const mi355rec_jaccard_result_t* result);

/* ROW UPDATES (the reference lists "Real-time Updates: Incremental index updates" among its extensions): songs are re-analysed
 * and corrected every day, and a changed row should not cost a rebuild of everything the handle keeps beside the rows.
 * mi355rec_update_rows changes `count` rows in place and returns once the update has been applied (synchronous, a set-up call
 * like the setters).  From then on every route of the handle and of every lane of its group answers exactly as a handle freshly
 * created from the updated matrix would: ids, order, score and distance bits.
 *   feats_host != NULL: count x 12 floats, row i for local_rows[i]; the matrix must be the library's own (mi355rec_create).  The rows
 *                       are written and everything derived from them is redone.
 *   feats_host == NULL: the caller has already changed those rows of the matrix (the borrowed matrix of mi355rec_create_device —
 *                       the writes complete before the call — or an owned one): only what is derived from them is redone.
 * What is exact afterwards, where the handle has it: the fp32 row, its entry in the fp16 and in the 8-bit replica, its norm
 * (distance requests) and its slot in the label-grouped copy of mi355rec_set_labels.  Priors, groups, row labels and row sets do
 * not depend on the features and stay.  Any fp32 values are accepted: zero, tiny, huge, infinite and NaN rows take the replicas'
 * special encodings, as at create.  Two snapshots only ever PLACE a bound and may stay stale without changing a result: the
 * anchor table (the caller's is recopied, a lane's is not) and the bucketed sample.  A stale one costs candidates, not
 * correctness: mi355rec_update_info_t::rows_since_snapshot counts the rows updated since the replicas were last built from all
 * rows (create, mi355rec_rebuild_replica: they reset it) and is the cue for an eventual rebuild.
 * INVALID_ARG (with a message), checked before anything is written: host rows on a borrowed matrix; a row outside [0, n); a row
 * named twice (two threads would race on one row); another lane of the group with a streamed query or batch open.
 * count == 0 succeeds and changes nothing.  An error AFTER the checks (a HIP error, out of memory; on a node handle, a failure on
 * one shard after others succeeded) may leave the update applied in part: repeating it with the same rows and features is safe.
 * LANES: the rows and the replicas are the group's, so an update through any member serves all of them.  Two rules: flush every
 * lane first (mi355rec_enqueue_flush: a stashed or pending streamed query carries a cutoff taken from the old rows; the caller's
 * own are completed by the call, another member's make it fail), and let no other thread use the group during the call.  What
 * the members have enqueued need not have finished: before its first write the call waits for every other member's own stream and
 * for the stream each was last used on, so work enqueued before the call is answered from the old rows, whole.  The
 * norms of the distance requests belong to each handle: the caller's are rewritten, the other members drop theirs and build
 * them again on their next distance request.
 * Device: no new kernel.  The update is a further job of q8_build_kernel (csrc/replica_q8.hip.h): thread e reads staged row e and
 * stores the row and its entries at row local_rows[e], through the packers the builders themselves call.  Rows are staged through
 * a pinned buffer of at most 65 536 rows; a larger update goes in chunks.
 * Node handle: feats_host is required (the node owns its rows; NULL is INVALID_ARG).  The open window is closed and the workers
 * are drained first; tickets waited for earlier stay readable.  A row-sharded placement gives each shard the rows it owns, a
 * replicated one applies the update once per device, the CPU backend rewrites its host matrix.
 * mi355rec_update_info: out->size = sizeof(mi355rec_update_info_t) of the caller's header on entry; no more than that is written.
 * mi355rec_replica_entries copies the stored entries of the given rows (any order, duplicates allowed) to the host: 24 B per row
 * of the fp16 replica, 12 B of the 8-bit one, and the norm where the handle has built norms (out_norms is left alone
 * otherwise).  Any out pointer may be NULL.  INVALID_ARG on a handle without replicas.  For tests: an updated handle against a
 * fresh one, byte for byte.
 * Measured on one MI355X at 10 M uniform rows with the replicas (tools/run_update_rows.py, profiles/r18_update_rows.json; host wall
 * time around the synchronous call, medians of five alternating runs): 1 row 0.06 ms, 1 000 rows 0.085 ms, 100 000 rows 0.50 ms,
 * 1 000 000 rows 4.5 ms (0.07 / 0.09 / 0.83 / 7.4 ms with labels set); beside it mi355rec_rebuild_replica 13.8 ms and destroying and
 * creating the handle again from host memory 65 ms (429 ms with the labels set again).  Staleness, streamed top-100 queries by row:
 * 21.88 us per query and 5 164 rows to the exact chain fresh, 21.90 us / 5 209 rows with 1 % of the rows updated, 21.97 us / 5 621
 * with 10 %, 21.87 us / 5 152 after mi355rec_rebuild_replica.  bench.py's headline against the parent commit, three alternating
 * runs each: 55 588 / 55 853 / 55 120 queries/s beside the parent's 54 936 ... 56 679 (profiles/r18_update_rows_ab.json).
 * Not served: appending or deleting rows (a deleted song is a row set); per-row updates of priors, labels or groups; an
 * incremental refresh of the bucketed sample; updates inside a running stream. */
typedef struct {
    uint32_t size;                /* in: sizeof of the caller's header                                           */
    float last_ms;                /* host wall time of the last mi355rec_update_rows call on this handle          */
    int64_t calls;                /* update calls on this handle that changed something, since create            */
    int64_t rows;                 /* rows they updated                                                           */
    int64_t rows_since_snapshot;  /* rows updated (through any lane of the group) since the replicas, the bucketed sample
                                     and the anchor tables were last built from all rows                          */
} mi355rec_update_info_t;         /* 32 bytes */
int mi355rec_update_rows(mi355rec_t* h, const int64_t* local_rows, int64_t count, const float* feats_host);
int mi355rec_sharded_update_rows(mi355rec_sharded_t* h, const int64_t* global_rows, int64_t count, const float* feats_host);
int mi355rec_update_info(const mi355rec_t* h, mi355rec_update_info_t* out);
int mi355rec_replica_entries(mi355rec_t* h, const int64_t* local_rows, int64_t count, void* out_half, void* out_q8, float* out_norms);

/* WHAT A NODE HANDLE IS MADE OF, for a companion library that serves it shard by shard (libmi355rec_embed.so,
 * include/mi355rec_embed.h).  Host-only accessors: nothing is launched or copied.
 * mi355rec_sharded_shard_handle: the single-device handle of shard `shard` (a replica of a replicated placement), owned by
 * the node handle and valid while it lives; the node's workers are drained first, and the caller must keep the node handle
 * itself idle while it uses the shard's.  INVALID_ARG on the CPU placement and for a shard that does not exist.
 * mi355rec_sharded_host_rows: the CPU placement's own row-major n x 12 host matrix — the LIVE one, which
 * mi355rec_sharded_update_rows rewrites in place.  INVALID_ARG on every other placement. */
int mi355rec_sharded_shard_handle(mi355rec_sharded_t* h, int shard, mi355rec_t** out);
int mi355rec_sharded_host_rows(const mi355rec_sharded_t* h, const float** rows, int64_t* n);

#ifdef MI355REC_TEST_HOOKS
/* TEST HOOK for the cross-workgroup hand-offs of the streamed scans (csrc/replica.hip.h, "hand-offs that fail
 * safe": sample values and cutoffs carry the epoch of their query, arrival counters are never reset).  Simulates
 * what a reader would see if the stores it depends on had not landed; results must stay those of the oracle —
 * only slower.  flags (or-ed):
 *   POISON          now (synchronises the device): every sample buffer and every left-behind cutoff of the handle is
 *                   overwritten with the most hostile values an EARLIER query could have left (a perfect score, a
 *                   cutoff of +1.0) under the epochs of the last queries;
 *   DROP_STORES     the next sampling launch (the seed riders of a streamed launch, or the sample launch of a batch on
 *                   its own / at the head of a stream) does not store the first half of its regions — riders that take the
 *                   BUCKETED sample store nothing at all — (whoever selects the cutoffs then reads whatever was there before);
 *   NO_LAST_RIDER   the next sampling launch is told a wrong arrival count, so none of its workgroups selects a cutoff
 *                   (the pass behind it then finds whatever cutoff was there before).
 * Never needed in production and NOT in the product library: declared and compiled only with -DMI355REC_TEST_HOOKS
 * (spotify_recommender_amd/build.py: libmi355rec_testhooks.so = the product's sources and flags + that define, the same
 * device code; tests/test_gpu_testhooks.py runs tests/test_gpu_replica.py and tests/test_gpu_half_multi.py against it). */
#define MI355REC_DEBUG_HANDOFF_POISON 1
#define MI355REC_DEBUG_HANDOFF_DROP_STORES 2
#define MI355REC_DEBUG_HANDOFF_NO_LAST_RIDER 4
int mi355rec_debug_handoff(mi355rec_t* h, int flags);
#endif /* MI355REC_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_DIAG_H */
