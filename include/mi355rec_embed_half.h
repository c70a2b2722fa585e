/*
 * mi355rec_embed_half.h — C-ABI of libmi355rec_embed_half.so, the THIRD companion library of libmi355rec.so:
 * HALF-PRECISION EMBEDDING TABLES.  A table exported as fp16 or bf16 is attached as it is: the device holds and reads
 * the 2 bytes per value the model produced, and every answer stays exact.
 *
 * THE CONTRACT.  A half table is n x d 16-bit words, d in {16, 32, 64, 128}, of one storage:
 *     MI355REC_EMBED_HALF_FP16   IEEE binary16
 *     MI355REC_EMBED_HALF_BF16   the upper 16 bits of an fp32
 * W(x) is the exact fp32 value of a stored word.  fp16: every finite value (subnormals included: 2^-24 widens to 2^-24,
 * never to 0) and inf map to the same real value, a NaN stays a NaN.  bf16: the fp32 whose bits are the word << 16.
 * Every answer — v and c of every row, ids, their order, the score bits, the count, the padding — is that of the
 * ARITHMETIC CONTRACT of mi355rec_embed.h with e_x = W(stored row x): the same tree, sqrtf, '/', clamp, blend and "no
 * key unless v is finite" rule, the same exclusion list, topn, metrics and audio side.  Nothing is added to that
 * contract and nothing of it is relaxed: widening is exact, every product is an fp32 product of widened values rounded
 * on its own, no mixed-precision or fused instruction takes part.
 *   A user formed from member rows is u = W(e_r0), then u = fl(u + W(e_rk)) in list order, in fp32.
 *   A user vector by value stays fp32.  The library never narrows anything: it takes the words as given (rounding an
 *   fp32 table to storage is the caller's choice; the Python layer offers it).
 *
 * The library has its own kernels (csrc/embed_half.hip.h) and reaches the catalogue as the first companion does:
 * mi355rec_stats (rows, row_base, device) and mi355rec_enqueue_scores (s(x), only when w_audio != 0).  It serves one
 * device handle.  Not served here: node handles and the CPU placement (libmi355rec_embed.so over the
 * widened table answers the same bits), user batches, half-precision user vectors, in-place table updates.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error, caller-owned buffers.  Calls are synchronous; one call
 * at a time per table; a table must be destroyed before its handle.  mi355rec_update_rows on the handle is seen by the
 * next hybrid call.  The query and result structs are mi355rec_embed.h's, read by the same size rule.
 */
#ifndef MI355REC_EMBED_HALF_H
#define MI355REC_EMBED_HALF_H

#include "mi355rec_embed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed_half mi355rec_embed_half_t;

#define MI355REC_EMBED_HALF_FP16 0
#define MI355REC_EMBED_HALF_BF16 1

typedef struct {
    uint32_t size;       /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;     /* device memory of the table (2 bytes per value) and its work buffers      */
    int32_t tile_rows;        /* rows of one tile of the scan                                              */
    int32_t grid;             /* workgroups of the scan                                                    */
    int32_t device;           /* HIP device of the handle                                                  */
    int32_t shards;           /* always 1                                                                  */
    int64_t queries;          /* _query and _scores calls served since create                              */
    int64_t scores_launches;  /* mi355rec_enqueue_scores launches they made (none with w_audio == 0)       */
    int32_t storage;          /* MI355REC_EMBED_HALF_FP16 / _BF16                                          */
    int32_t reserved;         /* 0                                                                         */
} mi355rec_embed_half_info_t;

/* table_words: row-major n x dim 16-bit words of `storage`, copied to the handle's device.  n must be the handle's rows. */
int mi355rec_embed_half_create(mi355rec_t* h, const uint16_t* table_words, int64_t n, int dim, int storage, mi355rec_embed_half_t** out);
void mi355rec_embed_half_destroy(mi355rec_embed_half_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_half_last_error(const mi355rec_embed_half_t* e);

int mi355rec_embed_half_query(mi355rec_embed_half_t* e, const mi355rec_embed_query_t* q, const mi355rec_embed_result_t* res);
/* The parity hook: v and c of EVERY row (rows floats each; out_c_host may be NULL).  topn, the exclusion list and the
 * result are not read. */
int mi355rec_embed_half_scores(mi355rec_embed_half_t* e, const mi355rec_embed_query_t* q, float* out_v_host, float* out_c_host);
int mi355rec_embed_half_info(const mi355rec_embed_half_t* e, mi355rec_embed_half_info_t* out);
/* A plain read of the table's bytes (the twin of mi355rec_embed_enqueue_probe): one checksum word per workgroup to
 * sink_dev (>= 1024 uint32). */
int mi355rec_embed_half_enqueue_probe(mi355rec_embed_half_t* e, uint32_t* sink_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_HALF_H */
