/*
 * mi355rec_embed_cand.h — C-ABI of libmi355rec_embed_cand.so, the SIXTH companion library of libmi355rec.so:
 * EMBEDDING CANDIDATE LISTS.  A request names the rows it is about — a list of up to 2^20 global ids in device memory, in
 * any order, with duplicates — and the library reads those rows of the table and nothing else: a gather of
 * n_candidates rows where every other request of the family is a pass over the whole table.  It is the second stage
 * of retrieval: an index or a first-stage model proposes, this ranks (enqueue_rank) or values (enqueue_scores) exactly.
 * The conventions are those of the fifth library (mi355rec_embed_stream.h): the table is fp32, fp16 or bf16 device
 * memory, borrowed or copied; every request input and output is device memory; a call runs on the CALLER's stream and
 * returns after launching.
 *
 * THE CONTRACT is by identity.  What mi355rec_embed_cand_enqueue_rank leaves in the result — ids, their order, the score
 * bits, the count, the -1 / 0 padding — is what mi355rec_embed_sets_query (include/mi355rec_embed_sets.h) writes for the
 * same user vector, audio side, exclusion list, metric, weights and topn when `only` is the set made of the listed ids
 * and there is no `seen` set: the top-N over the DISTINCT listed rows of the table.  A candidate id that is negative or
 * outside [row_base, row_base + rows) matches nothing, a row listed more than once is ranked once, excluded ids are left
 * out, a row whose v is not finite forms no key.  What mi355rec_embed_cand_enqueue_scores writes for list entry i is, bit
 * for bit, what mi355rec_embed_scores (fp32) or mi355rec_embed_half_scores (fp16 / bf16) writes for that row: v in
 * out_v_dev[i], c in out_c_dev[i], 1 in out_flag_dev[i] — in list order, duplicates included.  An id outside the table
 * gets the quiet NaN 0x7FC00000 in v and c and flag 0 (the rule of the audio engine's candidate scores).  The arithmetic
 * is mi355rec_embed.h's ARITHMETIC CONTRACT, by reference.
 *
 * AN ENQUEUE CALL launches and returns.  It neither waits for the device nor allocates nor copies from host memory: the
 * scalars of a request travel as kernel arguments, every work buffer was allocated at create.  The work buffers belong
 * to the table, so the library orders the calls of one table itself with the table's one event, as the fifth library
 * does.  A table may be used from several streams, by ONE host thread at a time.  A refused call launches nothing.
 *   The audio side (w_audio != 0) is mi355rec_enqueue_scores on the caller's stream into a buffer of one float per row of
 * the WHOLE catalogue, of which the gather then reads 4 bytes per listed row: that keeps the identity, and costs one
 * whole-catalogue audio launch (about 100 us at 10 M rows) however short the list is.
 *
 * Not served here: node handles and the CPU placement; user batches over a list, or one list per user;
 * row sets beside a list; a user formed from member rows; more than 2^20 candidates; the position in the list of each
 * ranked result; a gathered audio side; the C++ class and the CLI; graph capture.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error.  A table must be destroyed before its handle, and
 * destroy waits for the device.  Every pointer named *_dev is memory of the handle's device.
 */
#ifndef MI355REC_EMBED_CAND_H
#define MI355REC_EMBED_CAND_H

#include "mi355rec_embed_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed_cand mi355rec_embed_cand_t;

#define MI355REC_EMBED_CAND_MAX (1 << 20)   /* candidates per call: the audio engine's MI355REC_MAX_CANDIDATES */
#define MI355REC_EMBED_CAND_MAX_EXCLUDE 1024

/* The structs are self-sized by the rule of mi355rec_embed_query_t: `size` first, it must be the end of a field, a
 * shorter struct is read as "later fields zero", 0 or more than this library knows is refused. */

/* One user and one list.  The scalars are host values read at enqueue time. */
typedef struct {
    uint32_t size;
    uint32_t flags;                 /* must be 0 */
    const float* user_dev;          /* dim floats, 16-byte aligned                                                  */
    const float* audio;             /* 12 HOST floats read before the call returns, or NULL: audio_row is the audio */
                                    /* query (read only if w_audio != 0)                                            */
    const int64_t* candidates_dev;  /* n_candidates global ids, any order, duplicates allowed                       */
    const int64_t* exclude_dev;     /* n_exclude global ids (enqueue_rank only)                                     */
    int64_t audio_row;              /* a local row of the handle                                                    */
    int64_t n_candidates;           /* 0 .. MI355REC_EMBED_CAND_MAX                                                 */
    int32_t n_exclude;              /* 0 .. MI355REC_EMBED_CAND_MAX_EXCLUDE (enqueue_rank only)                     */
    int32_t topn;                   /* 1 .. MI355REC_MAX_TOPN_FAST (enqueue_rank only)                              */
    int32_t metric;                 /* MI355REC_EMBED_COSINE / _DOT                                                 */
    float w_audio;                  /* finite, |w| <= MI355REC_EMBED_MAX_WEIGHT                                     */
    float w_embed;                  /* the same, and not 0                                                          */
    uint32_t reserved;              /* must be 0 */
} mi355rec_embed_cand_query_t;

/* What enqueue_scores writes: n_candidates values each, in list order, all on the device. */
typedef struct {
    uint32_t size;
    uint32_t reserved;      /* must be 0 */
    float* out_v_dev;       /* v of every listed row; never NULL with n_candidates > 0 */
    float* out_c_dev;       /* c (the embedding term before its weight); may be NULL   */
    uint8_t* out_flag_dev;  /* 1: the id is a row of the table, 0: it is not; may be NULL */
} mi355rec_embed_cand_scores_t;

typedef struct {
    uint32_t size;            /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;     /* device memory this table allocated: its work buffers, and the table only if copied */
    int32_t tile_rows;        /* list entries of one tile of the gather (the rows of one tile of the scan)          */
    int32_t grid;             /* the most workgroups a gather takes (the single-user scan's grid)                   */
    int32_t device;           /* HIP device of the handle                                                           */
    int32_t storage;          /* MI355REC_EMBED_STREAM_FP32, MI355REC_EMBED_HALF_FP16 / _BF16                       */
    const void* table_dev;    /* the rows every gather reads (a borrowed table: the pointer given to create_device) */
    int64_t launches;         /* kernel launches enqueued since create (scores launches too)                        */
    int64_t enqueues;         /* enqueue calls accepted since create                                                */
    int64_t scores_launches;  /* mi355rec_enqueue_scores launches among them                                        */
    int32_t pass_users;       /* 1: a list is one user's                                                            */
    int32_t borrowed;         /* 1: the table is the caller's memory                                                */
    int32_t max_candidates;   /* MI355REC_EMBED_CAND_MAX                                                            */
    int32_t rank_launches;    /* launches of one enqueue_rank with a non-empty list, no exclusions and w_audio == 0 */
                              /* (claim, gather, merge, finish); an exclusion list and an audio side add one each   */
    int32_t scores_call_launches;  /* launches of one enqueue_scores with a non-empty list and w_audio == 0         */
    int32_t reserved;
} mi355rec_embed_cand_info_t;

/* table_dev: row-major n x dim values on the handle's device, 16-byte aligned, BORROWED: the caller keeps it alive until
 * destroy.  storage: MI355REC_EMBED_STREAM_FP32 (floats), MI355REC_EMBED_HALF_FP16 or _BF16 (16-bit words).  dim 16, 32, 64
 * or 128; n must be the handle's rows.  A handle on the CPU placement is refused. */
int mi355rec_embed_cand_create_device(mi355rec_t* h, const void* table_dev, int64_t n, int dim, int storage, mi355rec_embed_cand_t** out);
/* The same over a copy of host memory, for callers without a device tensor. */
int mi355rec_embed_cand_create(mi355rec_t* h, const void* table_host, int64_t n, int dim, int storage, mi355rec_embed_cand_t** out);
void mi355rec_embed_cand_destroy(mi355rec_embed_cand_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_cand_last_error(const mi355rec_embed_cand_t* e);
int mi355rec_embed_cand_info(const mi355rec_embed_cand_t* e, mi355rec_embed_cand_info_t* out);

/* stream: a hipStream_t (NULL: the null stream).  res is the fifth library's result: topn ids and scores and one count.
 * With n_candidates == 0 the count is 0 and everything is padding. */
int mi355rec_embed_cand_enqueue_rank(mi355rec_embed_cand_t* e, const mi355rec_embed_cand_query_t* q, const mi355rec_embed_stream_result_t* res,
                                     void* stream);
/* topn and the exclusion list of q are not read.  With n_candidates == 0 nothing is launched. */
int mi355rec_embed_cand_enqueue_scores(mi355rec_embed_cand_t* e, const mi355rec_embed_cand_query_t* q, const mi355rec_embed_cand_scores_t* res,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_CAND_H */
