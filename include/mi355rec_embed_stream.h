/*
 * mi355rec_embed_stream.h — C-ABI of libmi355rec_embed_stream.so, the FIFTH companion library of libmi355rec.so:
 * STREAMED EMBEDDING REQUESTS.  The table, the user vectors and the exclusion lists are device memory, every call runs on
 * the CALLER's stream and returns after launching, and the answer is left in device memory: no copy through the host, no
 * synchronise, no second copy of a table that a model already holds on the GPU.
 *
 * THE CONTRACT is by identity.  What mi355rec_embed_stream_enqueue_query leaves in the result — ids, their order, the
 * score bits, the count, the -1 / 0 padding — is what mi355rec_embed_query (include/mi355rec_embed.h) writes for the same
 * rows, user vector, audio side, exclusion list, metric, weights and topn; over fp16 / bf16 storage, what
 * mi355rec_embed_half_query (include/mi355rec_embed_half.h) writes.  What mi355rec_embed_stream_enqueue_users leaves for
 * user b is what mi355rec_embed_batch_query (include/mi355rec_embed_batch.h) writes for user b whose exclusion list is
 * row b of the matrix with its negative entries dropped.  The arithmetic is mi355rec_embed.h's ARITHMETIC CONTRACT, by
 * reference: the scans are the other libraries' scan bodies, compiled into this library.
 *
 * A BORROWED TABLE (mi355rec_embed_stream_create_device) is the caller's memory: nothing is copied, nothing is derived
 * from it and kept, nothing is freed at destroy.  Rows may be rewritten between enqueues in stream order; a request
 * enqueued after the write sees the new rows.  That is the in-place update of an embedding table.
 *
 * AN ENQUEUE CALL launches and returns.  It neither waits for the device nor allocates nor copies from host memory: the
 * scalars of a request travel as kernel arguments, every work buffer was allocated at create.  The work buffers belong
 * to the table, so the library orders the calls of one table itself: it records the table's one event behind every
 * enqueue and, when the next enqueue names another stream, makes that stream wait on the event (the host never does).
 * A table may be used from several streams, by ONE host thread at a time.  A refused call launches nothing.
 *   The audio side (w_audio != 0) is mi355rec_enqueue_scores on the caller's stream, by audio_row or by value: the 12
 * host floats of `audio` are read before the call returns (they travel as kernel arguments too) and never after.
 *
 * Not served here: row sets, half tables for user batches, more than 1024 exclusions per user, a user
 * formed from member rows, node handles and the CPU placement, the C++ class and the CLI; graph capture is untested.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error.  A table must be destroyed before its handle, and
 * destroy waits for the device.  Every pointer named *_dev is memory of the handle's device.
 */
#ifndef MI355REC_EMBED_STREAM_H
#define MI355REC_EMBED_STREAM_H

#include "mi355rec_embed_half.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed_stream mi355rec_embed_stream_t;

#define MI355REC_EMBED_STREAM_FP32 (-1)        /* `storage` of an fp32 table; else MI355REC_EMBED_HALF_FP16 / _BF16 */
#define MI355REC_EMBED_STREAM_MAX_EXCLUDE 1024 /* ids per user, on both paths                                       */
#define MI355REC_EMBED_STREAM_MAX_USERS 1024
#define MI355REC_EMBED_STREAM_MAX_USERS_TOPN 128

/* The structs are self-sized by the rule of mi355rec_embed_query_t: `size` first, it must be the end of a field, a
 * shorter struct is read as "later fields zero", 0 or more than this library knows is refused. */

/* One user.  The scalars are host values read at enqueue time. */
typedef struct {
    uint32_t size;
    uint32_t flags;              /* must be 0 */
    const float* user_dev;       /* dim floats, 16-byte aligned                                                     */
    const float* audio;          /* 12 HOST floats read before the call returns, or NULL: audio_row is the audio    */
                                 /* query (read only if w_audio != 0)                                               */
    const int64_t* exclude_dev;  /* n_exclude global ids, any order, duplicates allowed; a negative id or one       */
                                 /* outside [row_base, row_base + rows) matches nothing                             */
    int64_t audio_row;           /* a local row of the handle                                                       */
    int32_t n_exclude;           /* 0 .. MI355REC_EMBED_STREAM_MAX_EXCLUDE                                          */
    int32_t topn;                /* 1 .. MI355REC_MAX_TOPN_FAST                                                     */
    int32_t metric;              /* MI355REC_EMBED_COSINE / _DOT                                                    */
    float w_audio;               /* finite, |w| <= MI355REC_EMBED_MAX_WEIGHT                                        */
    float w_embed;               /* the same, and not 0                                                             */
    uint32_t reserved;           /* must be 0 */
} mi355rec_embed_stream_query_t;

/* Many users over an fp32 table. */
typedef struct {
    uint32_t size;
    uint32_t flags;              /* must be 0 */
    const float* users_dev;      /* n_users x dim floats, row-major, 16-byte aligned; no padding behind the last    */
    const int64_t* exclude_dev;  /* n_users x exclude_len global ids, row-major, a row padded with -1; or NULL with */
                                 /* exclude_len 0                                                                   */
    int32_t n_users;             /* 1 .. MI355REC_EMBED_STREAM_MAX_USERS                                            */
    int32_t topn;                /* 1 .. MI355REC_EMBED_STREAM_MAX_USERS_TOPN                                       */
    int32_t exclude_len;         /* L: 0 .. MI355REC_EMBED_STREAM_MAX_EXCLUDE                                       */
    int32_t metric;
    float w_embed;               /* finite, not 0, |w| <= MI355REC_EMBED_MAX_WEIGHT                                 */
    uint32_t reserved;           /* must be 0 */
} mi355rec_embed_stream_users_t;

/* Both calls: users x topn (one user: topn) ids and scores, users counts, all on the device. */
typedef struct {
    uint32_t size;
    uint32_t reserved;       /* must be 0 */
    int64_t* out_idx_dev;    /* global rows, -1 padded; never NULL */
    float* out_score_dev;    /* values v, 0 padded; may be NULL    */
    int32_t* out_count_dev;  /* may be NULL                        */
} mi355rec_embed_stream_result_t;

typedef struct {
    uint32_t size;            /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;     /* device memory this table allocated: its work buffers, and the table only if copied */
    int32_t tile_rows;        /* rows of one tile of the single-user scan                                           */
    int32_t grid;             /* workgroups of the single-user scan                                                 */
    int32_t device;           /* HIP device of the handle                                                           */
    int32_t storage;          /* MI355REC_EMBED_STREAM_FP32, MI355REC_EMBED_HALF_FP16 / _BF16                       */
    const void* table_dev;    /* the rows every scan reads (a borrowed table: the pointer given to create_device)   */
    int64_t launches;         /* kernel launches, copies and memsets enqueued since create (scores launches too)    */
    int64_t enqueues;         /* enqueue calls accepted since create                                                */
    int64_t scores_launches;  /* mi355rec_enqueue_scores launches among them                                        */
    int32_t pass_users;       /* users that share one pass of enqueue_users                                         */
    int32_t borrowed;         /* 1: the table is the caller's memory                                                */
} mi355rec_embed_stream_info_t;

/* table_dev: row-major n x dim values on the handle's device, 16-byte aligned, BORROWED: the caller keeps it alive until
 * destroy.  storage: MI355REC_EMBED_STREAM_FP32 (floats), MI355REC_EMBED_HALF_FP16 or _BF16 (16-bit words).  dim 16, 32, 64
 * or 128; n must be the handle's rows.  A handle on the CPU placement is refused. */
int mi355rec_embed_stream_create_device(mi355rec_t* h, const void* table_dev, int64_t n, int dim, int storage, mi355rec_embed_stream_t** out);
/* The same over a copy of host memory, for callers without a device tensor. */
int mi355rec_embed_stream_create(mi355rec_t* h, const void* table_host, int64_t n, int dim, int storage, mi355rec_embed_stream_t** out);
void mi355rec_embed_stream_destroy(mi355rec_embed_stream_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_stream_last_error(const mi355rec_embed_stream_t* e);
int mi355rec_embed_stream_info(const mi355rec_embed_stream_t* e, mi355rec_embed_stream_info_t* out);

/* stream: a hipStream_t (NULL: the null stream). */
int mi355rec_embed_stream_enqueue_query(mi355rec_embed_stream_t* e, const mi355rec_embed_stream_query_t* q,
                                        const mi355rec_embed_stream_result_t* res, void* stream);
int mi355rec_embed_stream_enqueue_users(mi355rec_embed_stream_t* e, const mi355rec_embed_stream_users_t* q,
                                        const mi355rec_embed_stream_result_t* res, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_STREAM_H */
