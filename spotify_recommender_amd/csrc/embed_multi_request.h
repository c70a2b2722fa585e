// embed_multi_request.h — what libmi355rec_embed_multi.so (include/mi355rec_embed_multi.h) reads on the host: its
// self-sized request and result with every refusal, and the plain C++ statements of the two rules its kernels add to the
// family's arithmetic (csrc/embed_multi.hip.h): THE VALUE (V = the largest finite v_k, the interest = the lowest k that
// gives it) and THE MERGE of identity 2 (K single-interest top-N lists into the one list a request leaves).  The table
// checks and the exclusion list are the stream library's (embed_stream_request.h).  Shared by the library
// (embed_multi.hip) and the stand-alone check (tests/embed_multi_check.cpp).  Host code only: no pointer named *_dev is
// ever read here.
#pragma once

#include <cstdint>

#include "embed_stream_request.h"   // invalid_table, invalid_metric_or_weight, prepare_width; read_sized' rule below it
#include "mi355rec_embed_multi.h"

namespace mi355embedmulti {

struct Query {
    const float* interests_dev = nullptr;   // n_interests x dim floats
    int n_interests = 0;
    const float* audio = nullptr;           // 12 HOST floats, or null with audio_row (read only with use_audio)
    int64_t audio_row = -1;
    const int64_t* exclude_dev = nullptr;
    int n_exclude = 0;
    int topn = 0;
    int metric = MI355REC_EMBED_COSINE;
    float w_audio = 0.0f;
    float w_embed = 0.0f;
    bool use_audio = false;
};

// True when the handle cannot carry a table: `device` is mi355rec_stats' (negative on the CPU placement).
inline bool invalid_handle(int device, char* msg, size_t cap) {
    if (device >= 0) return false;
    std::snprintf(msg, cap, "multi-interest embedding requests need a handle on a HIP device (the CPU placement is not served)");
    return true;
}

// The result, read by read_sized' rule and checked.
inline bool from_multi_result(const mi355rec_embed_multi_result_t* res, mi355rec_embed_multi_result_t* full_res, char* msg, size_t cap) {
    using R = mi355rec_embed_multi_result_t;
    static const size_t rends[] = {offsetof(R, reserved),      offsetof(R, out_idx_dev),      offsetof(R, out_score_dev),
                                   offsetof(R, out_count_dev), offsetof(R, out_interest_dev), sizeof(R)};
    static_assert(sizeof(R) == offsetof(R, out_interest_dev) + sizeof(int32_t*) && sizeof(R) == 40, "no tail padding");
    if (mi355playlist::read_sized(res, "embed multi result", rends, full_res, msg, cap)) return true;
    if (full_res->reserved != 0u) {
        std::snprintf(msg, cap, "reserved 0x%x in an embed multi result: must be 0", static_cast<unsigned>(full_res->reserved));
        return true;
    }
    return false;
}

// The request as the Query, read by read_sized' rule and checked; n_rows: the rows audio_row indexes.  True when it cannot
// be used; then msg[0..cap) says why (a refusal names the request's own fault first, then the result's).
inline bool from_multi_query(const mi355rec_embed_multi_query_t* q, const mi355rec_embed_multi_result_t* res, int64_t n_rows,
                             mi355rec_embed_multi_query_t* full, mi355rec_embed_multi_result_t* full_res, Query* r, char* msg, size_t cap) {
    using Q = mi355rec_embed_multi_query_t;
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Q, flags),     offsetof(Q, interests_dev), offsetof(Q, audio),     offsetof(Q, exclude_dev),
                                  offsetof(Q, audio_row), offsetof(Q, n_interests),   offsetof(Q, n_exclude), offsetof(Q, topn),
                                  offsetof(Q, metric),    offsetof(Q, w_audio),       offsetof(Q, w_embed),   offsetof(Q, reserved),
                                  sizeof(Q)};
    static_assert(sizeof(Q) == offsetof(Q, reserved) + sizeof(uint64_t) && sizeof(Q) == 72, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(q, "embed multi query", ends, full, msg, cap)) return true;
    if (from_multi_result(res, full_res, msg, cap)) return true;
    if (full->flags != 0u || full->reserved != 0u) {
        std::snprintf(msg, cap, "flags 0x%x / reserved 0x%llx in an embed multi query: must be 0", static_cast<unsigned>(full->flags),
                      static_cast<unsigned long long>(full->reserved));
        return true;
    }
    if (full->n_interests < 1 || full->n_interests > MI355REC_EMBED_MULTI_MAX_INTERESTS) {
        std::snprintf(msg, cap, "n_interests %d out of [1, %d]", static_cast<int>(full->n_interests), MI355REC_EMBED_MULTI_MAX_INTERESTS);
        return true;
    }
    if (!full->interests_dev) {
        std::snprintf(msg, cap, "null interests_dev in an embed multi query (interests by rows are not served: pass vectors)");
        return true;
    }
    if ((reinterpret_cast<uintptr_t>(full->interests_dev) & 15u) != 0u) {
        std::snprintf(msg, cap, "interests_dev is not 16-byte aligned");
        return true;
    }
    if (mi355embedstream::invalid_metric_or_weight("an embed multi query", full->metric, full->w_embed, msg, cap)) return true;
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
    if (full->topn < 1 || full->topn > MI355REC_MAX_TOPN_FAST) {
        std::snprintf(msg, cap, "topn %d out of [1, %d] (a multi-interest query has one round)", static_cast<int>(full->topn), MI355REC_MAX_TOPN_FAST);
        return true;
    }
    if (full->n_exclude < 0 || full->n_exclude > MI355REC_EMBED_MULTI_MAX_EXCLUDE) {
        std::snprintf(msg, cap, "n_exclude %d out of [0, %d]", static_cast<int>(full->n_exclude), MI355REC_EMBED_MULTI_MAX_EXCLUDE);
        return true;
    }
    if (full->n_exclude > 0 && !full->exclude_dev) {
        std::snprintf(msg, cap, "null exclusion list with n_exclude %d", static_cast<int>(full->n_exclude));
        return true;
    }
    if (!full_res->out_idx_dev) {
        std::snprintf(msg, cap, "null out_idx_dev in an embed multi result");
        return true;
    }
    r->interests_dev = full->interests_dev;
    r->n_interests = full->n_interests;
    r->audio = full->audio;
    r->audio_row = full->audio ? -1 : full->audio_row;
    r->exclude_dev = full->exclude_dev;
    r->n_exclude = full->n_exclude;
    r->topn = full->topn;
    r->metric = full->metric;
    r->w_audio = full->w_audio;
    r->w_embed = full->w_embed;
    r->use_audio = use_audio;
    return false;
}

// ---- THE VALUE, as embed_multi_scan_kernel and embed_multi_finish_kernel take it ----

// v[0 .. K): the contract's values of one row, one per interest.  False when none is finite (the row forms no key); else *V
// is the largest finite one and *interest the lowest k with v[k] == *V (a float comparison: -0.0 == +0.0, and the first of
// the two is the one kept — a key reports either as +0.0).
inline bool multi_value(const float* v, int K, float* V, int* interest) {
    bool have = false;
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(v[k])) continue;
        if (!have || v[k] > *V) {
            *V = v[k];
            *interest = k;
            have = true;
        }
    }
    return have;
}

// The ordered image of a value and the key of a row, as core.hip.h's pack_key forms them (restated: this header is host-only).
inline uint64_t key_of(float s, uint32_t global_row) {
    s = s + 0.0f;   // -0.0f -> +0.0f
    uint32_t u;
    std::memcpy(&u, &s, sizeof u);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (static_cast<uint64_t>(o) << 32) | static_cast<uint64_t>(~global_row);
}

// ---- THE MERGE of identity 2 ----

// keys[k * topn .. k * topn + counts[k]): the keys of interest k's single-interest result, sorted descending.  The union by
// row with the larger value kept and the lower k preferred at equal values, ordered by key, its first topn into out_keys /
// out_interest; returns how many.  (A row's keys differ only in the value's image, so "larger value" is "larger key".)
inline int merge_lists(const uint64_t* keys, const int* counts, int K, int topn, uint64_t* out_keys, int32_t* out_interest) {
    int head[MI355REC_EMBED_MULTI_MAX_INTERESTS] = {0};
    int n_out = 0;
    while (n_out < topn) {
        int best = -1;
        for (int k = 0; k < K; ++k)   // (strict: the lower k wins equal keys)
            if (head[k] < counts[k] && (best < 0 || keys[k * topn + head[k]] > keys[best * topn + head[best]])) best = k;
        if (best < 0) break;
        const uint64_t key = keys[best * topn + head[best]++];
        bool seen = false;   // (a row seen before was seen with a larger or equal value: the lists are taken in key order)
        for (int i = 0; i < n_out && !seen; ++i) seen = static_cast<uint32_t>(out_keys[i]) == static_cast<uint32_t>(key);
        if (seen) continue;
        out_keys[n_out] = key;
        out_interest[n_out] = best;
        ++n_out;
    }
    return n_out;
}

}  // namespace mi355embedmulti
