/*
 * mi355rec_embed_sets.h — C-ABI of libmi355rec_embed_sets.so, the FOURTH companion library of libmi355rec.so:
 * RESTRICTED EMBEDDING REQUESTS.  A hybrid request (mi355rec_embed.h) that leaves out a listening history of any
 * length (`seen`) and / or ranks only within a row set (`only`: a genre, a market, a candidate pool), exactly.
 *
 * THE CONTRACT.  A row is admissible iff it is admissible for mi355rec_embed_query (its v is finite and it is not in
 * exclude_global) AND (seen is NULL or the row is not in it) AND (only is NULL or the row is in it).  Everything else is
 * the ARITHMETIC CONTRACT of mi355rec_embed.h, over the widened values W(x) of mi355rec_embed_half.h for half storage,
 * bit for bit: v and c of a row, order, ties, -0.0 reported as +0.0, count = min(topn, admissible rows), the padding.
 * Member rows may lie inside or outside either set: the library does not exclude them.
 *   IDENTITIES.  No sets: the answer of mi355rec_embed_query / mi355rec_embed_half_query on the same table.  seen of at
 *   most 1024 rows: that call with the rows appended to exclude_global.  only holding every row, or seen empty: the plain
 *   answer.  only empty, seen holding every row, or only a subset of seen: count 0 — and where the host copies of the
 *   sets show it nothing is launched (launches_skipped).
 *
 * TABLES.  One table type over one device handle, in fp32, fp16 or bf16 storage; the library holds its own device copy.
 * ROW SETS.  One bit per row of the table (n / 8 bytes on the host and on the device), made from global ids or from a
 * mask of one byte per row (a label selection: labels == g, made by the caller).  Id rules are those of
 * mi355rec_rowset_* (mi355rec_diag.h): duplicates are allowed, in any order; ids outside [row_base, row_base + n) match
 * nothing; a negative id, a NULL list with n_ids > 0 and n_ids < 0 are INVALID_ARG; n_ids == 0 makes an empty set; a
 * failed add leaves the set unchanged.  Errors of create go to the table's last error, errors of add too.  A set belongs
 * to the table it was made on (a set of another table in a query is INVALID_ARG) and is destroyed before it.  create
 * and add copy to the device synchronously before they return; a query only reads a set.
 * THE SCAN (csrc/embed_sets.hip.h) tests the row's bit before a key is formed and does not load a tile (64 .. 1024
 * rows) in which no row is admissible by the sets: a catalogue grouped by genre costs one genre's rows, not the table.
 * tiles_scored / tiles_total count it.
 *
 * The library reaches the catalogue as the other companions do: mi355rec_stats and mi355rec_enqueue_scores.  Not served
 * here: node handles and the CPU placement, user batches, the parity hook and the probe (the first and
 * third companions have them over the same arithmetic), removing ids from a set, set algebra beyond only AND NOT seen,
 * the C++ class and the CLI.
 *
 * Conventions are mi355rec.h's: 0 = success, negative = error, caller-owned buffers.  Calls are synchronous; one call at
 * a time per table; a table must be destroyed before its handle.
 */
#ifndef MI355REC_EMBED_SETS_H
#define MI355REC_EMBED_SETS_H

#include "mi355rec_embed_half.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355rec_embed_sets mi355rec_embed_sets_t;
typedef struct mi355rec_embed_sets_rowset mi355rec_embed_sets_rowset_t;

/* Self-sized, read by the size rule of mi355rec_embed_query_t. */
typedef struct {
    uint32_t size;
    uint32_t flags;                             /* must be 0 */
    const mi355rec_embed_sets_rowset_t* seen;   /* NULL, or the rows to leave out   */
    const mi355rec_embed_sets_rowset_t* only;   /* NULL, or the rows to rank within */
} mi355rec_embed_sets_ext_t;

typedef struct {
    uint32_t size;       /* sizeof of this struct on entry */
    int32_t dim;
    int64_t rows;
    int64_t device_bytes;     /* device memory of the table, its work buffers and its live row sets        */
    int32_t tile_rows;        /* rows of one tile of the scan                                              */
    int32_t grid;             /* workgroups of the scan                                                    */
    int32_t device;           /* HIP device of the handle                                                  */
    int32_t shards;           /* always 1                                                                  */
    int64_t queries;          /* _query calls served since create                                          */
    int64_t scores_launches;  /* mi355rec_enqueue_scores launches they made (none with w_audio == 0)       */
    int32_t storage;          /* MI355REC_EMBED_HALF_FP16 / _BF16, -1 for fp32                             */
    int32_t reserved;         /* 0                                                                         */
    int64_t tiles_total;      /* tiles of the table, summed over all scan launches since create            */
    int64_t tiles_scored;     /* ... of which were loaded and scored                                       */
    int64_t launches_skipped; /* calls answered without a launch (the host bitmaps showed count 0)         */
} mi355rec_embed_sets_info_t;

/* table_host: row-major n x dim floats, copied to the handle's device.  n must be the handle's rows. */
int mi355rec_embed_sets_create(mi355rec_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_sets_t** out);
/* table_words: row-major n x dim 16-bit words of `storage` (MI355REC_EMBED_HALF_FP16 / _BF16). */
int mi355rec_embed_sets_create_half(mi355rec_t* h, const uint16_t* table_words, int64_t n, int dim, int storage, mi355rec_embed_sets_t** out);
void mi355rec_embed_sets_destroy(mi355rec_embed_sets_t* e);
/* The text of the last error of this table; with e == NULL, of the last failed create on this thread. */
const char* mi355rec_embed_sets_last_error(const mi355rec_embed_sets_t* e);
int mi355rec_embed_sets_info(const mi355rec_embed_sets_t* e, mi355rec_embed_sets_info_t* out);

int mi355rec_embed_sets_rowset_create(mi355rec_embed_sets_t* e, const int64_t* global_ids, int64_t n_ids, mi355rec_embed_sets_rowset_t** out);
/* mask_bytes: n bytes, one per row of the table (n must be its rows); non-zero means in the set. */
int mi355rec_embed_sets_rowset_create_mask(mi355rec_embed_sets_t* e, const uint8_t* mask_bytes, int64_t n, mi355rec_embed_sets_rowset_t** out);
int mi355rec_embed_sets_rowset_add(mi355rec_embed_sets_rowset_t* s, const int64_t* global_ids, int64_t n_ids);
/* The distinct rows of the table in the set; -1 for NULL. */
int64_t mi355rec_embed_sets_rowset_count(const mi355rec_embed_sets_rowset_t* s);
void mi355rec_embed_sets_rowset_destroy(mi355rec_embed_sets_rowset_t* s);   /* NULL is fine */

/* ext may be NULL (no sets), and so may either of its pointers. */
int mi355rec_embed_sets_query(mi355rec_embed_sets_t* e, const mi355rec_embed_query_t* q, const mi355rec_embed_sets_ext_t* ext,
                              const mi355rec_embed_result_t* res);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_EMBED_SETS_H */
