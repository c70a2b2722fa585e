// embed_request.h — ONE description of a hybrid request over an embedding table (include/mi355rec_embed.h), its argument
// checks and the host statement of its arithmetic, shared by the device tables (embed.hip), the CPU placement
// (embed_cpu.cpp) and the stand-alone check (tests/embed_check.cpp).  Host code only.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mi355rec_embed.h"
#include "playlist_request.h"   // read_sized: the size rule of every self-sized struct

namespace mi355embed {

struct Request {
    const float* user = nullptr;      // dim floats by value, or null with ...
    const int64_t* rows = nullptr;    // ... k checked rows of the table
    int k = 0;
    const float* audio = nullptr;     // 12 floats, or null with audio_row (read only with use_audio)
    int64_t audio_row = -1;
    const int64_t* exclude = nullptr;
    int n_exclude = 0;
    int topn = 0;
    int metric = MI355REC_EMBED_COSINE;
    float w_audio = 0.0f;
    float w_embed = 0.0f;
    bool use_audio = false;           // w_audio != 0: s(x) is read
};

inline bool valid_dim(int dim) { return dim == 16 || dim == 32 || dim == 64 || dim == 128; }

// True when table dimensions cannot be served; then msg[0..cap) says why.
inline bool invalid_table(const float* table, int64_t n, int dim, int64_t handle_rows, char* msg, size_t cap) {
    if (!valid_dim(dim)) {
        std::snprintf(msg, cap, "embedding dim %d: 16, 32, 64 or 128 are supported (zero-pad other widths)", dim);
        return true;
    }
    if (n != handle_rows) {
        std::snprintf(msg, cap, "table of %lld rows for a handle of %lld rows", static_cast<long long>(n),
                      static_cast<long long>(handle_rows));
        return true;
    }
    if (n > 0 && !table) {
        std::snprintf(msg, cap, "null table");
        return true;
    }
    return false;
}

// The C-ABI's query as the Request every layer takes, read by read_sized' rule and checked; n_rows: the rows that `rows`
// and `audio_row` index.  select: a _query call (topn, the exclusion list and the result are checked); false: a _scores call.
// True when it cannot be used; then msg[0..cap) says why.
inline bool from_query(const mi355rec_embed_query_t* q, const mi355rec_embed_result_t* res, bool select, int64_t n_rows,
                       mi355rec_embed_query_t* full, mi355rec_embed_result_t* full_res, Request* r, char* msg, size_t cap) {
    using Q = mi355rec_embed_query_t;
    using R = mi355rec_embed_result_t;
    if (!q || (select && !res)) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Q, flags), offsetof(Q, user), offsetof(Q, rows), offsetof(Q, audio), offsetof(Q, exclude_global),
                                  offsetof(Q, audio_row), offsetof(Q, k), offsetof(Q, n_exclude), offsetof(Q, topn), offsetof(Q, metric),
                                  offsetof(Q, w_audio), offsetof(Q, w_embed), sizeof(Q)};
    static_assert(sizeof(Q) == offsetof(Q, w_embed) + sizeof(float) && sizeof(Q) == 72, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(q, "embed query", ends, full, msg, cap)) return true;
    if (select) {
        static const size_t rends[] = {offsetof(R, reserved), offsetof(R, out_idx), offsetof(R, out_score), offsetof(R, out_count), sizeof(R)};
        static_assert(sizeof(R) == offsetof(R, out_count) + sizeof(int*) && sizeof(R) == 32, "no tail padding");
        if (mi355playlist::read_sized(res, "embed result", rends, full_res, msg, cap)) return true;
        if (!full_res->out_idx) {
            std::snprintf(msg, cap, "null out_idx in an embed result");
            return true;
        }
    }
    if (full->flags != 0u) {
        std::snprintf(msg, cap, "flags 0x%x in an embed query: must be 0", static_cast<unsigned>(full->flags));
        return true;
    }
    if (full->user && full->rows) {
        std::snprintf(msg, cap, "user by value and by rows in one embed query");
        return true;
    }
    if (!full->user && !full->rows) {
        std::snprintf(msg, cap, "an embed query needs user by value or by rows");
        return true;
    }
    if (full->rows && (full->k < 1 || full->k > MI355REC_EMBED_MAX_MEMBERS)) {
        std::snprintf(msg, cap, "%d member rows: 1 to %d are supported", static_cast<int>(full->k), MI355REC_EMBED_MAX_MEMBERS);
        return true;
    }
    if (full->metric != MI355REC_EMBED_COSINE && full->metric != MI355REC_EMBED_DOT) {
        std::snprintf(msg, cap, "metric %d in an embed query: MI355REC_EMBED_COSINE (0) or MI355REC_EMBED_DOT (1)", static_cast<int>(full->metric));
        return true;
    }
    if (!(std::fabs(full->w_embed) <= MI355REC_EMBED_MAX_WEIGHT) || full->w_embed == 0.0f) {   // (false for NaN)
        std::snprintf(msg, cap, "embed_weight %g: finite, not 0 and at most %g in magnitude", static_cast<double>(full->w_embed),
                      static_cast<double>(MI355REC_EMBED_MAX_WEIGHT));
        return true;
    }
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
    if (select) {
        if (full->topn < 1 || full->topn > MI355REC_MAX_TOPN_FAST) {
            std::snprintf(msg, cap, "topn %d out of [1, %d] (an embed query has one round)", static_cast<int>(full->topn), MI355REC_MAX_TOPN_FAST);
            return true;
        }
        if (full->n_exclude < 0 || full->n_exclude > MI355REC_EMBED_MAX_EXCLUDE) {
            std::snprintf(msg, cap, "n_exclude %d out of [0, %d]", static_cast<int>(full->n_exclude), MI355REC_EMBED_MAX_EXCLUDE);
            return true;
        }
        if (full->n_exclude > 0 && !full->exclude_global) {
            std::snprintf(msg, cap, "null exclusion list with n_exclude %d", static_cast<int>(full->n_exclude));
            return true;
        }
    }
    if (full->rows)
        for (int m = 0; m < full->k; ++m)
            if (full->rows[m] < 0 || full->rows[m] >= n_rows) {
                std::snprintf(msg, cap, "Invalid song index: %lld", static_cast<long long>(full->rows[m]));
                return true;
            }
    r->user = full->user;
    r->rows = full->rows;
    r->k = full->rows ? full->k : 0;
    r->audio = full->audio;
    r->audio_row = full->audio ? -1 : full->audio_row;
    r->exclude = select ? full->exclude_global : nullptr;
    r->n_exclude = select ? full->n_exclude : 0;
    r->topn = full->topn;
    r->metric = full->metric;
    r->w_audio = full->w_audio;
    r->w_embed = full->w_embed;
    r->use_audio = use_audio;
    return false;
}

// ---- the arithmetic contract on the host (include/mi355rec_embed.h) — compile with -ffp-contract=off ----

// tree(a, b): group partials of four, then pairwise levels.
inline float tree(const float* a, const float* b, int d) {
    float t[MI355REC_EMBED_MAX_DIM / 4];
    int m = d / 4;
    for (int g = 0; g < m; ++g) {
        float p = a[4 * g] * b[4 * g];
        p = p + a[4 * g + 1] * b[4 * g + 1];
        p = p + a[4 * g + 2] * b[4 * g + 2];
        p = p + a[4 * g + 3] * b[4 * g + 3];
        t[g] = p;
    }
    for (; m > 1; m >>= 1)
        for (int g = 0; g < m / 2; ++g) t[g] = t[2 * g] + t[2 * g + 1];
    return t[0];
}

// c of one row: e the row, u the user vector, nu = sqrtf(tree(u, u)).
inline float similarity(const float* e, const float* u, float nu, int d, int metric) {
    const float dot = tree(e, u, d);
    if (metric == MI355REC_EMBED_DOT) return dot;
    const float den = std::sqrt(tree(e, e, d)) * nu;
    float c = 0.0f;
    if (den > 1e-8f) {
        const float t = dot / den;
        const float m = (t < 1.0f) ? t : 1.0f;
        c = (-1.0f < m) ? m : -1.0f;
    }
    return c;
}

// v of one row from its s and c.
inline float blend(const Request& r, float s, float c) {
    const float b = r.w_embed * c;
    if (!r.use_audio) return b;
    const float a = r.w_audio * s;
    return a + b;
}

// u of a request by rows: the element-wise sum in list order (fetch(row, out): the table's row).
template <class Fetch>
inline void sum_members(const Request& r, int d, Fetch fetch, float* u) {
    float e[MI355REC_EMBED_MAX_DIM];
    for (int m = 0; m < r.k; ++m) {
        fetch(r.rows[m], e);
        for (int j = 0; j < d; ++j) u[j] = m == 0 ? e[j] : u[j] + e[j];
    }
}

inline uint64_t key_of(float v, uint32_t global_row) {
    return (static_cast<uint64_t>(mi355playlist::ordered_image(v)) << 32) | static_cast<uint64_t>(static_cast<uint32_t>(~global_row));
}

// n sorted (descending) keys into the result: idx / score / count, padded to topn.
inline void write_result(const uint64_t* keys, int n, int topn, const mi355rec_embed_result_t& res) {
    for (int i = 0; i < topn; ++i) {
        const bool have = i < n;
        res.out_idx[i] = have ? static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(keys[i]))) : -1;
        if (res.out_score) {
            float s = 0.0f;
            if (have) {
                const uint32_t o = static_cast<uint32_t>(keys[i] >> 32);
                const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
                std::memcpy(&s, &u, sizeof s);
            }
            res.out_score[i] = s;
        }
    }
    if (res.out_count) *res.out_count = n;
}

}  // namespace mi355embed

// ---- the CPU placement (embed_cpu.cpp): the same contract over host memory, rows split over OpenMP threads ----
namespace mi355embed {

struct CpuTable {
    const float* table = nullptr;        // n x dim, row-major
    int64_t n = 0;
    int dim = 0;
    const float* audio_rows = nullptr;   // the catalogue's LIVE n x 12 host matrix (mi355rec_sharded_host_rows)
};

// v (and c, unless out_c is null) of every row.
void cpu_scores(const CpuTable& t, const Request& r, float* out_v, float* out_c);
// The request's top-N into res (padded).  False: out of host memory.
bool cpu_query(const CpuTable& t, const Request& r, const mi355rec_embed_result_t& res);

}  // namespace mi355embed
