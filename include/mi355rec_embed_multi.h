/*
 * mi355rec_embed_multi.h — C-ABI of libmi355rec_embed_multi.so, the SEVENTH companion library of libmi355rec.so:
 * MULTI-INTEREST EMBEDDING REQUESTS.  A multi-interest user model (several user heads, several learned interests) hands
 * the retriever K vectors for ONE user and wants ONE list: the rows that match any of the interests best, and which
 * interest that was.  One call reads the table once for all K interests, keeps one candidate list, and leaves the top-N
 * by the best interest with its attribution.  The conventions are those of the fifth library (mi355rec_embed_stream.h):
 * the table is fp32, fp16 or bf16 device memory, borrowed or copied; every request input and output is device memory; a
 * call runs on the CALLER's stream and returns after launching.
 *
 * THE CONTRACT, by arithmetic.  Let v_k(x) be what mi355rec_embed.h's ARITHMETIC CONTRACT gives row x with u = interest k
 * (over half storage: applied to the widened values).  A row forms a key iff some v_k(x) is finite; its value is
 * V(x) = max over the finite v_k(x); its interest is the LOWEST k with v_k(x) == V(x) — a float comparison, so -0.0 equals
 * +0.0, and the value is reported as +0.0 (as every key of the family reports it).  Keys, exclusions, the count and the
 * -1 / 0 padding are the contract's.
 *
 * THE CONTRACT, by identity.
 *   1. K = 1.  With n_interests == 1 the result is, bit for bit, what mi355rec_embed_stream_enqueue_query leaves for that
 *      vector; out_interest is 0 for every result.
 *   2. Any K.  The result is the merge of the K results of mi355rec_embed_stream_enqueue_query, one per interest, with the
 *      same topn, exclusions, audio side and weights: union by row, keep the larger value, prefer the lower k at equal
 *      values, order by key (value descending, then id ascending), keep the first topn.  The identity is exact: a row in the
 *      top-N by V has V = v_k for some k, every row ahead of it in list k is ahead of it by V too, so it is within that
 *      list's top-N.
 *
 * AN ENQUEUE CALL launches and returns.  It neither waits for the device nor allocates nor copies from host memory: the
 * scalars of a request travel as kernel arguments, every work buffer was allocated at create, and the interests are read
 * where the caller left them (they must stay valid, in stream order, until the call's work has run).  The work buffers
 * belong to the table, so the library orders the calls of one table itself with the table's one event, as the fifth
 * library does.  A table may be used from several streams, by ONE host thread at a time.  A refused call launches nothing.
 *   The audio side (w_audio != 0) is mi355rec_enqueue_scores on the caller's stream, by audio_row or by value: it is one
 * audio query for all interests.
 *
 * Not served here: per-interest weights or quotas; row sets or candidate lists beside interests; interests
 * formed from member rows; batches of multi-interest users; node handles and the CPU placement; the C++ class and the CLI;
 * graph capture.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error.  A table must be destroyed before its handle, and
 * destroy waits for the device.  Every pointer named *_dev is memory of the handle's device.
 */
#ifndef MI355REC_EMBED_MULTI_H
#define MI355REC_EMBED_MULTI_H

#include "mi355rec_embed_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed_multi mi355rec_embed_multi_t;

#define MI355REC_EMBED_MULTI_MAX_INTERESTS 32   /* the family's MAX_MEMBERS */
#define MI355REC_EMBED_MULTI_MAX_EXCLUDE 1024

/* The structs are self-sized by the rule of mi355rec_embed_query_t: `size` first, it must be the end of a field, a
 * shorter struct is read as "later fields zero", 0 or more than this library knows is refused. */

/* One user of n_interests vectors.  The scalars are host values read at enqueue time. */
typedef struct {
    uint32_t size;
    uint32_t flags;              /* must be 0 */
    const float* interests_dev;  /* n_interests x dim floats, row-major, 16-byte aligned                            */
    const float* audio;          /* 12 HOST floats read before the call returns, or NULL: audio_row is the audio    */
                                 /* query (read only if w_audio != 0)                                               */
    const int64_t* exclude_dev;  /* n_exclude global ids, any order, duplicates allowed; a negative id or one       */
                                 /* outside [row_base, row_base + rows) matches nothing                             */
    int64_t audio_row;           /* a local row of the handle                                                       */
    int32_t n_interests;         /* 1 .. MI355REC_EMBED_MULTI_MAX_INTERESTS                                         */
    int32_t n_exclude;           /* 0 .. MI355REC_EMBED_MULTI_MAX_EXCLUDE                                           */
    int32_t topn;                /* 1 .. MI355REC_MAX_TOPN_FAST                                                     */
    int32_t metric;              /* MI355REC_EMBED_COSINE / _DOT                                                    */
    float w_audio;               /* finite, |w| <= MI355REC_EMBED_MAX_WEIGHT                                        */
    float w_embed;               /* the same, and not 0                                                             */
    uint64_t reserved;           /* must be 0 */
} mi355rec_embed_multi_query_t;

/* The stream library's result and the attribution: topn ids, scores and interests and one count, all on the device. */
typedef struct {
    uint32_t size;
    uint32_t reserved;          /* must be 0 */
    int64_t* out_idx_dev;       /* global rows, -1 padded; never NULL                                    */
    float* out_score_dev;       /* values V, 0 padded; may be NULL                                       */
    int32_t* out_count_dev;     /* may be NULL                                                           */
    int32_t* out_interest_dev;  /* the interest that gave the row its value, -1 padded; may be NULL      */
} mi355rec_embed_multi_result_t;

typedef struct {
    uint32_t size;            /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;     /* device memory this table allocated: its work buffers, and the table only if copied */
    int32_t tile_rows;        /* rows of one tile of the scan                                                       */
    int32_t grid;             /* workgroups of the scan                                                             */
    int32_t device;           /* HIP device of the handle                                                           */
    int32_t storage;          /* MI355REC_EMBED_STREAM_FP32, MI355REC_EMBED_HALF_FP16 / _BF16                       */
    const void* table_dev;    /* the rows every scan reads (a borrowed table: the pointer given to create_device)   */
    int64_t launches;         /* kernel launches enqueued since create (scores launches too)                        */
    int64_t enqueues;         /* enqueue calls accepted since create                                                */
    int64_t scores_launches;  /* mi355rec_enqueue_scores launches among them                                        */
    int32_t pass_users;       /* 1: a request is one user's                                                         */
    int32_t borrowed;         /* 1: the table is the caller's memory                                                */
    int32_t max_interests;    /* MI355REC_EMBED_MULTI_MAX_INTERESTS                                                 */
    int32_t pass_interests;   /* interests the scan holds in registers at a time (its compile-time chunk width)     */
    int32_t query_launches;   /* launches of one request with no exclusions and w_audio == 0 (scan, merge, finish); */
                              /* an exclusion list and an audio side add one each                                   */
    int32_t reserved;
} mi355rec_embed_multi_info_t;

/* table_dev: row-major n x dim values on the handle's device, 16-byte aligned, BORROWED: the caller keeps it alive until
 * destroy.  storage: MI355REC_EMBED_STREAM_FP32 (floats), MI355REC_EMBED_HALF_FP16 or _BF16 (16-bit words).  dim 16, 32, 64
 * or 128; n must be the handle's rows.  A handle on the CPU placement is refused. */
int mi355rec_embed_multi_create_device(mi355rec_t* h, const void* table_dev, int64_t n, int dim, int storage, mi355rec_embed_multi_t** out);
/* The same over a copy of host memory, for callers without a device tensor. */
int mi355rec_embed_multi_create(mi355rec_t* h, const void* table_host, int64_t n, int dim, int storage, mi355rec_embed_multi_t** out);
void mi355rec_embed_multi_destroy(mi355rec_embed_multi_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_multi_last_error(const mi355rec_embed_multi_t* e);
int mi355rec_embed_multi_info(const mi355rec_embed_multi_t* e, mi355rec_embed_multi_info_t* out);

/* stream: a hipStream_t (NULL: the null stream). */
int mi355rec_embed_multi_enqueue_query(mi355rec_embed_multi_t* e, const mi355rec_embed_multi_query_t* q, const mi355rec_embed_multi_result_t* res,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_MULTI_H */
