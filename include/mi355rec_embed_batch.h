/*
 * mi355rec_embed_batch.h — C-ABI of libmi355rec_embed_batch.so, the SECOND companion library of libmi355rec.so: USER
 * BATCHES over an embedding table.  B users are answered by ceil(B / pass_users) passes over the table instead of B:
 * the users of one pass share every 16-byte load, the row's squared norm and its square root.
 *
 * THE CONTRACT.  For every user b of a call, ids, their order, the score bits and the count are exactly those of
 * mi355rec_embed_query (include/mi355rec_embed.h) with user = users[b], w_audio = 0 and the same metric, w_embed, topn
 * and that user's exclusion list.  The arithmetic is that header's ARITHMETIC CONTRACT, by reference: nothing is added
 * to it and nothing of it is relaxed (fp32 tree sums, no FMA, correctly rounded sqrtf and '/').  A user whose every v is
 * not finite gets count 0.  The users of one pass never influence each other.
 *
 * The library has its own kernels (csrc/embed_batch.hip.h) and its OWN device copy of the table; it reaches the
 * catalogue only through mi355rec_stats (rows, row_base, device).  Not served here: an audio side
 * (w_audio != 0), node handles and the CPU placement, topn > 128, asynchronous calls, a table shared with
 * libmi355rec_embed.so.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error, caller-owned buffers.  Calls are synchronous; one call
 * at a time per table; a table must be destroyed before its handle.
 */
#ifndef MI355REC_EMBED_BATCH_H
#define MI355REC_EMBED_BATCH_H

#include "mi355rec_embed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed_batch mi355rec_embed_batch_t;

#define MI355REC_EMBED_BATCH_MAX_USERS 1024
#define MI355REC_EMBED_BATCH_MAX_TOPN 128
#define MI355REC_EMBED_BATCH_MAX_EXCLUDE 65536

/* Self-sized by the rule of mi355rec_embed_query_t: `size` first, it must be the end of a field, a shorter struct is read
 * as "later fields zero", 0 or more than this library knows is refused. */
typedef struct {
    uint32_t size;
    uint32_t flags;                  /* must be 0 */
    const float* users;              /* n_users x dim floats, row-major                                                  */
    const int64_t* exclude_global;   /* the users' exclusion lists, one after the other (global ids), or NULL with ...  */
    const int64_t* exclude_offsets;  /* ... n_users + 1 non-decreasing offsets into it (CSR): user b's list is            */
                                     /* [offsets[b], offsets[b+1]).  Both NULL: nothing is excluded.  Duplicates are       */
                                     /* allowed, ids outside the handle's rows match nothing; at most                      */
                                     /* MI355REC_EMBED_BATCH_MAX_EXCLUDE ids per user.                                     */
    int32_t n_users;                 /* 1 .. MI355REC_EMBED_BATCH_MAX_USERS                                              */
    int32_t topn;                    /* 1 .. MI355REC_EMBED_BATCH_MAX_TOPN                                               */
    int32_t metric;                  /* MI355REC_EMBED_COSINE / _DOT                                                     */
    float w_embed;                   /* finite, not 0, |w| <= MI355REC_EMBED_MAX_WEIGHT                                  */
} mi355rec_embed_batch_query_t;

typedef struct {
    uint32_t size;
    uint32_t reserved;    /* must be 0 */
    int64_t* out_idx;     /* n_users x topn global rows, -1 padded; never NULL */
    float* out_score;     /* n_users x topn values v, 0 padded; may be NULL    */
    int32_t* out_count;   /* n_users counts; may be NULL                       */
} mi355rec_embed_batch_result_t;

typedef struct {
    uint32_t size;          /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;   /* device memory of the table and the work buffers                          */
    int32_t tile_rows;      /* rows of one tile of the scan                                              */
    int32_t grid;           /* workgroups of the scan                                                    */
    int32_t device;         /* HIP device of the handle                                                  */
    int32_t pass_users;     /* users that share one pass over the table at this table's dim             */
    int64_t passes;         /* scan launches since create                                                */
    int64_t users_served;   /* users answered since create                                               */
} mi355rec_embed_batch_info_t;

/* table_host: row-major n x dim floats (dim 16, 32, 64 or 128), copied to the handle's device.  n must be the handle's rows. */
int mi355rec_embed_batch_create(mi355rec_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_batch_t** out);
void mi355rec_embed_batch_destroy(mi355rec_embed_batch_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_batch_last_error(const mi355rec_embed_batch_t* e);
int mi355rec_embed_batch_query(mi355rec_embed_batch_t* e, const mi355rec_embed_batch_query_t* q, const mi355rec_embed_batch_result_t* res);
int mi355rec_embed_batch_info(const mi355rec_embed_batch_t* e, mi355rec_embed_batch_info_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_BATCH_H */
