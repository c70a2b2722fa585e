// embed_cand_request.h — what libmi355rec_embed_cand.so (include/mi355rec_embed_cand.h) reads on the host: its self-sized
// request and the two results with their checks, and the plain C++ statements of the two steps its own kernels take in
// front of the arithmetic (csrc/embed_cand.hip.h): the ID MAPPING (a global id into a local row or the no-row word, the
// stream library's local_row) and the CLAIM (one list entry per distinct in-table row keeps its row, every other entry
// becomes the no-row word; the bitmap is all zero again once the owners have cleared their words).  The table checks, the
// result of a rank call and the exclusion list are the stream library's (embed_stream_request.h).  Shared by the library
// (embed_cand.hip) and the stand-alone check (tests/embed_cand_check.cpp).  Host code only: no pointer named *_dev is ever
// read here.
#pragma once

#include <cstdint>

#include "embed_stream_request.h"   // from_stream_result, invalid_table, local_row, kNoRow; read_sized' rule below it
#include "mi355rec_embed_cand.h"

namespace mi355embedcand {

using mi355embedstream::kNoRow;
using mi355embedstream::local_row;

struct Query {
    const float* user_dev = nullptr;
    const float* audio = nullptr;       // 12 HOST floats, or null with audio_row (read only with use_audio)
    int64_t audio_row = -1;
    const int64_t* candidates_dev = nullptr;
    int64_t n_candidates = 0;
    const int64_t* exclude_dev = nullptr;   // (a scores call: null, 0)
    int n_exclude = 0;
    int topn = 0;                           // (a scores call: 0)
    int metric = MI355REC_EMBED_COSINE;
    float w_audio = 0.0f;
    float w_embed = 0.0f;
    bool use_audio = false;
};

// The request as the Query, read by read_sized' rule and checked; n_rows: the rows audio_row indexes; rank: topn and the
// exclusion list are read (enqueue_rank) or left alone (enqueue_scores).  True when it cannot be used; then msg[0..cap) says why.
inline bool from_cand_query(const mi355rec_embed_cand_query_t* q, int64_t n_rows, bool rank, mi355rec_embed_cand_query_t* full, Query* r, char* msg,
                            size_t cap) {
    using Q = mi355rec_embed_cand_query_t;
    static const size_t ends[] = {offsetof(Q, flags), offsetof(Q, user_dev), offsetof(Q, audio), offsetof(Q, candidates_dev), offsetof(Q, exclude_dev),
                                  offsetof(Q, audio_row), offsetof(Q, n_candidates), offsetof(Q, n_exclude), offsetof(Q, topn), offsetof(Q, metric),
                                  offsetof(Q, w_audio), offsetof(Q, w_embed), offsetof(Q, reserved), sizeof(Q)};
    static_assert(sizeof(Q) == offsetof(Q, reserved) + sizeof(uint32_t) && sizeof(Q) == 80, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(q, "embed cand query", ends, full, msg, cap)) return true;
    if (full->flags != 0u || full->reserved != 0u) {
        std::snprintf(msg, cap, "flags 0x%x / reserved 0x%x in an embed cand query: must be 0", static_cast<unsigned>(full->flags),
                      static_cast<unsigned>(full->reserved));
        return true;
    }
    if (!full->user_dev) {
        std::snprintf(msg, cap, "null user_dev in an embed cand query (members by rows are not served: pass a vector)");
        return true;
    }
    if ((reinterpret_cast<uintptr_t>(full->user_dev) & 15u) != 0u) {
        std::snprintf(msg, cap, "user_dev is not 16-byte aligned");
        return true;
    }
    if (full->n_candidates < 0 || full->n_candidates > MI355REC_EMBED_CAND_MAX) {
        std::snprintf(msg, cap, "n_candidates %lld out of [0, %d]", static_cast<long long>(full->n_candidates), MI355REC_EMBED_CAND_MAX);
        return true;
    }
    if (full->n_candidates > 0 && !full->candidates_dev) {
        std::snprintf(msg, cap, "null candidate list with n_candidates %lld", static_cast<long long>(full->n_candidates));
        return true;
    }
    if (mi355embedstream::invalid_metric_or_weight("an embed cand query", full->metric, full->w_embed, msg, cap)) return true;
    if (!(std::fabs(full->w_audio) <= MI355REC_EMBED_MAX_WEIGHT)) {
        std::snprintf(msg, cap, "audio_weight %g: finite and at most %g in magnitude", static_cast<double>(full->w_audio),
                      static_cast<double>(MI355REC_EMBED_MAX_WEIGHT));
        return true;
    }
    const bool use_audio = full->w_audio != 0.0f;
    if (use_audio && !full->audio && (full->audio_row < 0 || full->audio_row >= n_rows)) {
        std::snprintf(msg, cap, "audio_weight %g needs audio by value or a valid audio_row, got row %lld", static_cast<double>(full->w_audio),
                      static_cast<long long>(full->audio_row));
        return true;
    }
    if (rank) {
        if (full->topn < 1 || full->topn > MI355REC_MAX_TOPN_FAST) {
            std::snprintf(msg, cap, "topn %d out of [1, %d] (a candidate list has one round)", static_cast<int>(full->topn), MI355REC_MAX_TOPN_FAST);
            return true;
        }
        if (full->n_exclude < 0 || full->n_exclude > MI355REC_EMBED_CAND_MAX_EXCLUDE) {
            std::snprintf(msg, cap, "n_exclude %d out of [0, %d]", static_cast<int>(full->n_exclude), MI355REC_EMBED_CAND_MAX_EXCLUDE);
            return true;
        }
        if (full->n_exclude > 0 && !full->exclude_dev) {
            std::snprintf(msg, cap, "null exclusion list with n_exclude %d", static_cast<int>(full->n_exclude));
            return true;
        }
    }
    r->user_dev = full->user_dev;
    r->audio = full->audio;
    r->audio_row = full->audio ? -1 : full->audio_row;
    r->candidates_dev = full->candidates_dev;
    r->n_candidates = full->n_candidates;
    r->exclude_dev = rank ? full->exclude_dev : nullptr;
    r->n_exclude = rank ? full->n_exclude : 0;
    r->topn = rank ? full->topn : 0;
    r->metric = full->metric;
    r->w_audio = full->w_audio;
    r->w_embed = full->w_embed;
    r->use_audio = use_audio;
    return false;
}

// A rank call: the request, then the stream library's result (a refusal names the request's own fault first).
inline bool from_cand_rank(const mi355rec_embed_cand_query_t* q, const mi355rec_embed_stream_result_t* res, int64_t n_rows,
                           mi355rec_embed_cand_query_t* full, mi355rec_embed_stream_result_t* full_res, Query* r, char* msg, size_t cap) {
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    if (from_cand_query(q, n_rows, true, full, r, msg, cap)) return true;
    if (mi355embedstream::from_stream_result(res, full_res, msg, cap)) return true;
    return mi355embedstream::null_out_idx(*full_res, msg, cap);
}

// A scores call: the request, then where the values go.
inline bool from_cand_scores(const mi355rec_embed_cand_query_t* q, const mi355rec_embed_cand_scores_t* res, int64_t n_rows,
                             mi355rec_embed_cand_query_t* full, mi355rec_embed_cand_scores_t* full_res, Query* r, char* msg, size_t cap) {
    using R = mi355rec_embed_cand_scores_t;
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    if (from_cand_query(q, n_rows, false, full, r, msg, cap)) return true;
    static const size_t rends[] = {offsetof(R, reserved), offsetof(R, out_v_dev), offsetof(R, out_c_dev), offsetof(R, out_flag_dev), sizeof(R)};
    static_assert(sizeof(R) == offsetof(R, out_flag_dev) + sizeof(uint8_t*) && sizeof(R) == 32, "no tail padding");
    if (mi355playlist::read_sized(res, "embed cand scores", rends, full_res, msg, cap)) return true;
    if (full_res->reserved != 0u) {
        std::snprintf(msg, cap, "reserved 0x%x in an embed cand scores result: must be 0", static_cast<unsigned>(full_res->reserved));
        return true;
    }
    if (r->n_candidates > 0 && !full_res->out_v_dev) {
        std::snprintf(msg, cap, "null out_v_dev with n_candidates %lld", static_cast<long long>(r->n_candidates));
        return true;
    }
    return false;
}

// ---- the CLAIM, as embed_cand_claim_kernel takes it (there the entries run concurrently: which copy of a row keeps it
// varies, that exactly one does, does not) ----

// 32-bit words of the claim bitmap of a table of n rows.
inline int64_t claim_words(int64_t n) { return (n + 31) / 32; }

// ids[0 .. m) into rows_out[0 .. m): an id outside the table becomes kNoRow; of the entries that name one row, the first
// to find the row's bit clear sets it and keeps the row, the others become kNoRow.  bitmap: claim_words(n) words, all zero
// on entry.
inline void claim_list(const int64_t* ids, int64_t m, int64_t row_base, int64_t n, uint32_t* bitmap, uint32_t* rows_out) {
    for (int64_t i = 0; i < m; ++i) {
        uint32_t local = local_row(ids[i], row_base, n);
        if (local != kNoRow) {
            const uint32_t bit = 1u << (local & 31u);
            if (bitmap[local >> 5] & bit) local = kNoRow;
            else bitmap[local >> 5] |= bit;
        }
        rows_out[i] = local;
    }
}

// What the gather's owners do behind the claim: every entry that kept a row stores 0 over the word that holds its bit.
// Every set bit has an owner, so the bitmap is all zero again.
inline void clear_claims(const uint32_t* rows, int64_t m, uint32_t* bitmap) {
    for (int64_t i = 0; i < m; ++i)
        if (rows[i] != kNoRow) bitmap[rows[i] >> 5] = 0u;
}

// Workgroups of a gather over m >= 1 entries: one per tile of the list, at most the scan's grid.
inline int gather_grid(int64_t m, int tile_entries, int scan_grid) {
    const int64_t tiles = (m + tile_entries - 1) / tile_entries;
    return static_cast<int>(tiles < scan_grid ? tiles : scan_grid);
}

}  // namespace mi355embedcand
