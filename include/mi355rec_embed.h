/*
 * mi355rec_embed.h — C-ABI of libmi355rec_embed.so, the COMPANION library of libmi355rec.so: EMBEDDING TABLES, the
 * hybrid model the reference lists among its extensions ("add collaborative filtering").
 *
 * A table holds a second vector per row of a handle: an embedding learned from who listens to what (matrix
 * factorisation, item2vec, a two-tower model), dim floats.  One request ranks EVERY row x of the handle by
 *
 *     v(x) = w_audio * (audio cosine of row x) + w_embed * (embedding similarity of row x)
 *
 * exactly, selected on the device, bit for bit equal to the CPU statement of the arithmetic below
 * (tests/embed_oracle.py).  The companion library has its own kernels (csrc/embed.hip) and reaches the catalogue only
 * through the C-ABI of libmi355rec.so: mi355rec_stats (rows, row_base, device), mi355rec_enqueue_scores (the audio
 * cosine of every row, into device memory, on the table's stream) and the two host-only accessors of the node handle
 * (mi355rec_sharded_shard_handle, mi355rec_sharded_host_rows).  Nothing in the product library's device code changes.
 *
 * THE ARITHMETIC CONTRACT (compiled with -ffp-contract=off: every product and every sum is rounded on its own, no FMA).
 *   dim d in {16, 32, 64, 128} (callers zero-pad other widths up to the next of these: a zero column changes no sum).
 *   TREE SUM tree(a, b) of two d-vectors:
 *       p_g     = fl(fl(fl(a[4g] b[4g] + a[4g+1] b[4g+1]) + a[4g+2] b[4g+2]) + a[4g+3] b[4g+3])     g = 0 .. d/4 - 1
 *       t^0_g   = p_g,   t^(l+1)_g = fl(t^l_(2g) + t^l_(2g+1))   until one value is left
 *     (layout-free: d/4 lanes with xor-butterflies produce it, and so does one thread in registers).
 *   dot = tree(e_x, u), nn = tree(e_x, e_x), nu = sqrtf(tree(u, u)); sqrtf and '/' correctly rounded.
 *   MI355REC_EMBED_COSINE:  den = fl(sqrtf(nn) * nu);  den > 1e-8f ?  c = t < 1 ? t : 1, then -1 < c ? c : -1 with
 *                           t = dot / den (the clamp of the audio chain)  :  c = 0.
 *   MI355REC_EMBED_DOT:     c = dot (what matrix-factorisation models score by).
 *   u is `user` (d floats by value) or the sum of k <= MI355REC_EMBED_MAX_MEMBERS rows of the table, element-wise:
 *       u = e_(r0), then u = fl(u + e_(rk)) in list order.
 *   s(x) is the score mi355rec_query_topn gives row x for the audio query (`audio`: 12 floats, or `audio_row`), bit for bit.
 *   v = fl(fl(w_audio * s) + fl(w_embed * c));  with w_audio == 0: v = fl(w_embed * c), and the audio rows are never read.
 *   Keys are mi355rec_pack_key(v, global row): v descending, then row ascending, -0.0 ranked and reported as +0.0.
 *   A row whose v is not finite forms no key (it is never returned).
 *   Excluded: the at most MI355REC_EMBED_MAX_EXCLUDE global ids of exclude_global (duplicates allowed; ids outside the
 *   handle's rows match nothing).  Member rows are NOT excluded by the library (the Python layer adds them by default).
 *   count = min(topn, rows that form a key and are not excluded); out_idx / out_score are padded with -1 / 0.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error, caller-owned buffers.  Calls are synchronous; one call
 * at a time per table; a table must be destroyed before its handle.  mi355rec_update_rows on the handle is seen by
 * the next hybrid call (the audio side reads the live matrix).  Updating the table in place is not served: destroy
 * and create.  The caller of a node-handle table must have no node-handle call in flight.
 */
#ifndef MI355REC_EMBED_H
#define MI355REC_EMBED_H

#include "mi355rec_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed mi355rec_embed_t;

#define MI355REC_EMBED_COSINE 0
#define MI355REC_EMBED_DOT 1
#define MI355REC_EMBED_MAX_DIM 128
#define MI355REC_EMBED_MAX_MEMBERS 32
#define MI355REC_EMBED_MAX_EXCLUDE 1024
#define MI355REC_EMBED_MAX_WEIGHT 4.0f

/* Self-sized (the rule of the playlist request): `size` = sizeof of the struct the caller compiled with; it must be the end
 * of a field; a shorter struct is read as "later fields zero"; 0 or more than this library knows is refused. */
typedef struct {
    uint32_t size;
    uint32_t flags;                 /* must be 0 */
    const float* user;              /* dim floats by value, or NULL with ...                                        */
    const int64_t* rows;            /* ... k rows of the table (local rows of a handle, global rows of a node handle) */
    const float* audio;             /* 12 floats, or NULL: audio_row is the audio query (read only if w_audio != 0)  */
    const int64_t* exclude_global;  /* n_exclude global ids                                                          */
    int64_t audio_row;              /* a row of the handle (local / global as `rows`)                                */
    int32_t k;
    int32_t n_exclude;
    int32_t topn;                   /* 1 .. MI355REC_MAX_TOPN_FAST                                                   */
    int32_t metric;                 /* MI355REC_EMBED_COSINE / _DOT                                                  */
    float w_audio;                  /* finite, |w| <= MI355REC_EMBED_MAX_WEIGHT                                      */
    float w_embed;                  /* the same, and not 0 (w_embed == 0 is the engine's own call)                   */
} mi355rec_embed_query_t;

typedef struct {
    uint32_t size;
    uint32_t reserved;   /* must be 0 */
    int64_t* out_idx;    /* topn global rows, -1 padded; never NULL */
    float* out_score;    /* topn values v, 0 padded; may be NULL    */
    int* out_count;      /* may be NULL                              */
} mi355rec_embed_result_t;

typedef struct {
    uint32_t size;       /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;     /* device memory of the table and its work buffers (0 on the CPU placement)  */
    int32_t tile_rows;        /* rows of one tile of the scan (0 on the CPU placement)                      */
    int32_t grid;             /* workgroups of the scan (the first shard's; 0 on the CPU placement)         */
    int32_t device;           /* HIP device of the first shard, -1 on the CPU placement                     */
    int32_t shards;           /* tables under this one: 1, or the shards of a row-sharded node handle       */
    int64_t queries;          /* _query and _scores calls served since create                               */
    int64_t scores_launches;  /* mi355rec_enqueue_scores launches they made (none with w_audio == 0)        */
} mi355rec_embed_info_t;

/* table_host: row-major n x dim floats, copied to the handle's device.  n must be the handle's rows. */
int mi355rec_embed_create(mi355rec_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_t** out);
/* The same over a node handle: a CPU placement is served on the host (csrc/embed_cpu.cpp: OpenMP, the same contract); a
 * row-sharded placement gets one table per shard over its slice and the shards' keys are merged on the host (exact: keys
 * carry v); a replicated placement is served by its first replica. */
int mi355rec_embed_create_node(mi355rec_sharded_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_t** out);
void mi355rec_embed_destroy(mi355rec_embed_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_last_error(const mi355rec_embed_t* e);

int mi355rec_embed_query(mi355rec_embed_t* e, const mi355rec_embed_query_t* q, const mi355rec_embed_result_t* res);
/* The parity hook, the twin of mi355rec_scores: v and c of EVERY row (rows floats each; out_c_host may be NULL).  topn,
 * the exclusion list and the result are not read (topn may be 0). */
int mi355rec_embed_scores(mi355rec_embed_t* e, const mi355rec_embed_query_t* q, float* out_v_host, float* out_c_host);
int mi355rec_embed_info(const mi355rec_embed_t* e, mi355rec_embed_info_t* out);
/* A plain read of the table (the twin of mi355rec_enqueue_stream_probe): one checksum word per workgroup to sink_dev
 * (>= 1024 uint32).  A table over one device handle only. */
int mi355rec_embed_enqueue_probe(mi355rec_embed_t* e, uint32_t* sink_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_H */
