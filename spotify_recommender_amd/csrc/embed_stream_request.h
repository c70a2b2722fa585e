// embed_stream_request.h — what libmi355rec_embed_stream.so (include/mi355rec_embed_stream.h) reads on the host: its two
// self-sized requests and the result, by read_sized' rule, with their checks, the create checks, and the plain C++
// statements of the two steps its own kernels take (csrc/embed_stream.hip.h): PREPARE (global ids into the sorted local
// rows the scans search) and FINISH (merged keys into ids, scores and a count).  Shared by the library (embed_stream.hip)
// and the stand-alone check (tests/embed_stream_check.cpp).  Host code only: no pointer named *_dev is ever read here.
#pragma once

#include <cstdint>

#include "embed_half_request.h"   // valid_storage; embed_request.h: read_sized' rule, valid_dim, write_result
#include "mi355rec_embed_stream.h"

namespace mi355embedstream {

struct Query {
    const float* user_dev = nullptr;
    const float* audio = nullptr;       // 12 HOST floats, or null with audio_row (read only with use_audio)
    int64_t audio_row = -1;
    const int64_t* exclude_dev = nullptr;
    int n_exclude = 0;
    int topn = 0;
    int metric = MI355REC_EMBED_COSINE;
    float w_audio = 0.0f;
    float w_embed = 0.0f;
    bool use_audio = false;
};

struct Users {
    const float* users_dev = nullptr;   // n_users x dim floats
    int n_users = 0;
    const int64_t* exclude_dev = nullptr;   // n_users x exclude_len, or null
    int exclude_len = 0;
    int topn = 0;
    int metric = MI355REC_EMBED_COSINE;
    float w_embed = 0.0f;
};

constexpr uint32_t kNoRow = 0xFFFFFFFFu;   // above every local row: what an id that matches nothing becomes

inline bool valid_storage(int storage) { return storage == MI355REC_EMBED_STREAM_FP32 || mi355embedhalf::valid_storage(storage); }

// True when a table cannot be served; then msg[0..cap) says why.  `table` is never read (device memory, or a host copy's source).
inline bool invalid_table(const void* table, int64_t n, int dim, int storage, int64_t handle_rows, bool borrowed, char* msg, size_t cap) {
    if (!valid_storage(storage)) {
        std::snprintf(msg, cap, "storage %d: MI355REC_EMBED_STREAM_FP32 (-1), MI355REC_EMBED_HALF_FP16 (0) or MI355REC_EMBED_HALF_BF16 (1)", storage);
        return true;
    }
    if (!mi355embed::valid_dim(dim)) {
        std::snprintf(msg, cap, "embedding dim %d: 16, 32, 64 or 128 are supported (zero-pad other widths)", dim);
        return true;
    }
    if (n != handle_rows) {
        std::snprintf(msg, cap, "table of %lld rows for a handle of %lld rows", static_cast<long long>(n), static_cast<long long>(handle_rows));
        return true;
    }
    if (n > 0 && !table) {
        std::snprintf(msg, cap, "null table");
        return true;
    }
    if (borrowed && (reinterpret_cast<uintptr_t>(table) & 15u) != 0u) {
        std::snprintf(msg, cap, "a borrowed table is 16-byte aligned (the scans load 16 bytes at a time)");
        return true;
    }
    return false;
}

// The result of either call, read and checked.
inline bool from_stream_result(const mi355rec_embed_stream_result_t* res, mi355rec_embed_stream_result_t* full_res, char* msg, size_t cap) {
    using R = mi355rec_embed_stream_result_t;
    static const size_t rends[] = {offsetof(R, reserved), offsetof(R, out_idx_dev), offsetof(R, out_score_dev), offsetof(R, out_count_dev), sizeof(R)};
    static_assert(sizeof(R) == offsetof(R, out_count_dev) + sizeof(int32_t*) && sizeof(R) == 32, "no tail padding");
    if (mi355playlist::read_sized(res, "embed stream result", rends, full_res, msg, cap)) return true;
    if (full_res->reserved != 0u) {
        std::snprintf(msg, cap, "reserved 0x%x in an embed stream result: must be 0", static_cast<unsigned>(full_res->reserved));
        return true;
    }
    return false;
}

// ... and what is asked of it once the request itself has passed (a refusal names the request's own fault first).
inline bool null_out_idx(const mi355rec_embed_stream_result_t& full_res, char* msg, size_t cap) {
    if (full_res.out_idx_dev) return false;
    std::snprintf(msg, cap, "null out_idx_dev in an embed stream result");
    return true;
}

inline bool invalid_metric_or_weight(const char* what, int metric, float w_embed, char* msg, size_t cap) {
    if (metric != MI355REC_EMBED_COSINE && metric != MI355REC_EMBED_DOT) {
        std::snprintf(msg, cap, "metric %d in %s: MI355REC_EMBED_COSINE (0) or MI355REC_EMBED_DOT (1)", metric, what);
        return true;
    }
    if (!(std::fabs(w_embed) <= MI355REC_EMBED_MAX_WEIGHT) || w_embed == 0.0f) {   // (false for NaN)
        std::snprintf(msg, cap, "embed_weight %g: finite, not 0 and at most %g in magnitude", static_cast<double>(w_embed),
                      static_cast<double>(MI355REC_EMBED_MAX_WEIGHT));
        return true;
    }
    return false;
}

// The one-user request as the Query, read by read_sized' rule and checked; n_rows: the rows audio_row indexes.  True when it
// cannot be used; then msg[0..cap) says why.
inline bool from_stream_query(const mi355rec_embed_stream_query_t* q, const mi355rec_embed_stream_result_t* res, int64_t n_rows,
                              mi355rec_embed_stream_query_t* full, mi355rec_embed_stream_result_t* full_res, Query* r, char* msg, size_t cap) {
    using Q = mi355rec_embed_stream_query_t;
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Q, flags), offsetof(Q, user_dev), offsetof(Q, audio), offsetof(Q, exclude_dev), offsetof(Q, audio_row),
                                  offsetof(Q, n_exclude), offsetof(Q, topn), offsetof(Q, metric), offsetof(Q, w_audio), offsetof(Q, w_embed),
                                  offsetof(Q, reserved), sizeof(Q)};
    static_assert(sizeof(Q) == offsetof(Q, reserved) + sizeof(uint32_t) && sizeof(Q) == 64, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(q, "embed stream query", ends, full, msg, cap)) return true;
    if (from_stream_result(res, full_res, msg, cap)) return true;
    if (full->flags != 0u || full->reserved != 0u) {
        std::snprintf(msg, cap, "flags 0x%x / reserved 0x%x in an embed stream query: must be 0", static_cast<unsigned>(full->flags),
                      static_cast<unsigned>(full->reserved));
        return true;
    }
    if (!full->user_dev) {
        std::snprintf(msg, cap, "null user_dev in an embed stream query (members by rows are not served: pass a vector)");
        return true;
    }
    if ((reinterpret_cast<uintptr_t>(full->user_dev) & 15u) != 0u) {
        std::snprintf(msg, cap, "user_dev is not 16-byte aligned");
        return true;
    }
    if (invalid_metric_or_weight("an embed stream query", full->metric, full->w_embed, msg, cap)) return true;
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
        std::snprintf(msg, cap, "topn %d out of [1, %d] (an embed query has one round)", static_cast<int>(full->topn), MI355REC_MAX_TOPN_FAST);
        return true;
    }
    if (full->n_exclude < 0 || full->n_exclude > MI355REC_EMBED_STREAM_MAX_EXCLUDE) {
        std::snprintf(msg, cap, "n_exclude %d out of [0, %d]", static_cast<int>(full->n_exclude), MI355REC_EMBED_STREAM_MAX_EXCLUDE);
        return true;
    }
    if (full->n_exclude > 0 && !full->exclude_dev) {
        std::snprintf(msg, cap, "null exclusion list with n_exclude %d", static_cast<int>(full->n_exclude));
        return true;
    }
    if (null_out_idx(*full_res, msg, cap)) return true;
    r->user_dev = full->user_dev;
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

// The many-user request as the Users, read by read_sized' rule and checked.
inline bool from_stream_users(const mi355rec_embed_stream_users_t* q, const mi355rec_embed_stream_result_t* res, mi355rec_embed_stream_users_t* full,
                              mi355rec_embed_stream_result_t* full_res, Users* r, char* msg, size_t cap) {
    using Q = mi355rec_embed_stream_users_t;
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Q, flags), offsetof(Q, users_dev), offsetof(Q, exclude_dev), offsetof(Q, n_users), offsetof(Q, topn),
                                  offsetof(Q, exclude_len), offsetof(Q, metric), offsetof(Q, w_embed), offsetof(Q, reserved), sizeof(Q)};
    static_assert(sizeof(Q) == offsetof(Q, reserved) + sizeof(uint32_t) && sizeof(Q) == 48, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(q, "embed stream users", ends, full, msg, cap)) return true;
    if (from_stream_result(res, full_res, msg, cap)) return true;
    if (full->flags != 0u || full->reserved != 0u) {
        std::snprintf(msg, cap, "flags 0x%x / reserved 0x%x in an embed stream users request: must be 0", static_cast<unsigned>(full->flags),
                      static_cast<unsigned>(full->reserved));
        return true;
    }
    if (full->n_users < 1 || full->n_users > MI355REC_EMBED_STREAM_MAX_USERS) {
        std::snprintf(msg, cap, "n_users %d out of [1, %d]", static_cast<int>(full->n_users), MI355REC_EMBED_STREAM_MAX_USERS);
        return true;
    }
    if (!full->users_dev) {
        std::snprintf(msg, cap, "null users_dev in an embed stream users request");
        return true;
    }
    if ((reinterpret_cast<uintptr_t>(full->users_dev) & 15u) != 0u) {
        std::snprintf(msg, cap, "users_dev is not 16-byte aligned");
        return true;
    }
    if (full->topn < 1 || full->topn > MI355REC_EMBED_STREAM_MAX_USERS_TOPN) {
        std::snprintf(msg, cap, "topn %d out of [1, %d] (a user batch has one round)", static_cast<int>(full->topn), MI355REC_EMBED_STREAM_MAX_USERS_TOPN);
        return true;
    }
    if (full->exclude_len < 0 || full->exclude_len > MI355REC_EMBED_STREAM_MAX_EXCLUDE) {
        std::snprintf(msg, cap, "exclude_len %d out of [0, %d]", static_cast<int>(full->exclude_len), MI355REC_EMBED_STREAM_MAX_EXCLUDE);
        return true;
    }
    if (full->exclude_len > 0 && !full->exclude_dev) {
        std::snprintf(msg, cap, "null exclusion matrix with exclude_len %d", static_cast<int>(full->exclude_len));
        return true;
    }
    if (invalid_metric_or_weight("an embed stream users request", full->metric, full->w_embed, msg, cap)) return true;
    if (null_out_idx(*full_res, msg, cap)) return true;
    r->users_dev = full->users_dev;
    r->n_users = full->n_users;
    r->exclude_dev = full->exclude_len > 0 ? full->exclude_dev : nullptr;
    r->exclude_len = full->exclude_len;
    r->topn = full->topn;
    r->metric = full->metric;
    r->w_embed = full->w_embed;
    return false;
}

// ---- PREPARE, as embed_stream_prepare_kernel takes it ----

// A global id as a local row of a table of n rows from row_base on, or kNoRow (compared before the subtraction can overflow).
inline uint32_t local_row(int64_t id, int64_t row_base, int64_t n) {
    if (id < 0 || id < row_base || id - row_base >= n) return kNoRow;
    return static_cast<uint32_t>(id - row_base);
}

// The threads of the sort: the next power of two from L on, and at least one wave.
inline int prepare_width(int L) {
    int w = 64;
    while (w < L) w <<= 1;
    return w;
}

// ids[0 .. L) into out[0 .. L): mapped, padded with kNoRow to prepare_width(L), sorted ascending by the bitonic network in
// the kernel's order of steps (element t against element t ^ j), the first L words kept.  L <= 1024.
inline void prepare_list(const int64_t* ids, int L, int64_t row_base, int64_t n, uint32_t* out) {
    uint32_t v[MI355REC_EMBED_STREAM_MAX_EXCLUDE], w[MI355REC_EMBED_STREAM_MAX_EXCLUDE];
    const int width = prepare_width(L);
    for (int t = 0; t < width; ++t) v[t] = t < L ? local_row(ids[t], row_base, n) : kNoRow;
    for (int k = 2; k <= width; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = 0; t < width; ++t) {
                const uint32_t other = v[t ^ j];
                const bool keep_min = ((t & k) == 0) == ((t & j) == 0);
                w[t] = keep_min ? (v[t] < other ? v[t] : other) : (v[t] < other ? other : v[t]);
            }
            std::memcpy(v, w, sizeof(uint32_t) * static_cast<size_t>(width));
        }
    for (int t = 0; t < L; ++t) out[t] = v[t];
}

// Is `local` in the sorted list, as both scan bodies ask (embed.hip.h, embed_batch.hip.h): a lower bound, then equality.
inline bool excluded(const uint32_t* list, int L, uint32_t local) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < local) lo = mid + 1;
        else hi = mid;
    }
    return lo < L && list[lo] == local;
}

// ---- FINISH, as embed_stream_finish_kernel takes it ----

// eff merged keys (sorted descending, 0 behind the last) into idx / score [topn] and *count: count = the non-zero keys, the
// decoding and the -1 / 0 padding of write_result.  score and count may be null.
inline void finish_keys(const uint64_t* keys, int eff, int topn, int64_t* idx, float* score, int32_t* count) {
    int c = 0;
    for (int i = 0; i < eff; ++i) c += keys[i] != 0ull ? 1 : 0;
    for (int i = 0; i < topn; ++i) {
        const bool have = i < c;
        idx[i] = have ? static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(keys[i]))) : -1;
        if (score) {
            float s = 0.0f;
            if (have) {
                const uint32_t o = static_cast<uint32_t>(keys[i] >> 32);
                const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
                std::memcpy(&s, &u, sizeof s);
            }
            score[i] = s;
        }
    }
    if (count) *count = c;
}

}  // namespace mi355embedstream
