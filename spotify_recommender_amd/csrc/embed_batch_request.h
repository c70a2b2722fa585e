// embed_batch_request.h — ONE description of a batch of users over an embedding table (include/mi355rec_embed_batch.h): its
// argument checks and the exclusion lists as the scan wants them, shared by the device table (embed_batch.hip) and the
// stand-alone check (tests/embed_batch_check.cpp).  Host code only.
#pragma once

#include <algorithm>
#include <vector>

#include "embed_request.h"   // read_sized' rule, valid_dim, invalid_table, write_result
#include "mi355rec_embed_batch.h"

namespace mi355embed {

struct BatchRequest {
    const float* users = nullptr;             // n_users x dim floats
    int n_users = 0;
    const int64_t* exclude = nullptr;         // global ids, or null with ...
    const int64_t* exclude_offsets = nullptr; // ... n_users + 1 checked offsets (both null: nothing excluded)
    int topn = 0;
    int metric = MI355REC_EMBED_COSINE;
    float w_embed = 0.0f;
};

// The C-ABI's structs as the BatchRequest, read by read_sized' rule and checked.  True when they cannot be used; then
// msg[0..cap) says why.
inline bool from_batch_query(const mi355rec_embed_batch_query_t* q, const mi355rec_embed_batch_result_t* res, mi355rec_embed_batch_query_t* full,
                             mi355rec_embed_batch_result_t* full_res, BatchRequest* r, char* msg, size_t cap) {
    using Q = mi355rec_embed_batch_query_t;
    using R = mi355rec_embed_batch_result_t;
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Q, flags), offsetof(Q, users), offsetof(Q, exclude_global), offsetof(Q, exclude_offsets), offsetof(Q, n_users),
                                  offsetof(Q, topn), offsetof(Q, metric), offsetof(Q, w_embed), sizeof(Q)};
    static_assert(sizeof(Q) == offsetof(Q, w_embed) + sizeof(float) && sizeof(Q) == 48, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(q, "embed batch query", ends, full, msg, cap)) return true;
    static const size_t rends[] = {offsetof(R, reserved), offsetof(R, out_idx), offsetof(R, out_score), offsetof(R, out_count), sizeof(R)};
    static_assert(sizeof(R) == offsetof(R, out_count) + sizeof(int32_t*) && sizeof(R) == 32, "no tail padding");
    if (mi355playlist::read_sized(res, "embed batch result", rends, full_res, msg, cap)) return true;
    if (!full_res->out_idx) {
        std::snprintf(msg, cap, "null out_idx in an embed batch result");
        return true;
    }
    if (full->flags != 0u) {
        std::snprintf(msg, cap, "flags 0x%x in an embed batch query: must be 0", static_cast<unsigned>(full->flags));
        return true;
    }
    if (full->n_users < 1 || full->n_users > MI355REC_EMBED_BATCH_MAX_USERS) {
        std::snprintf(msg, cap, "n_users %d out of [1, %d]", static_cast<int>(full->n_users), MI355REC_EMBED_BATCH_MAX_USERS);
        return true;
    }
    if (!full->users) {
        std::snprintf(msg, cap, "null users in an embed batch query");
        return true;
    }
    if (full->topn < 1 || full->topn > MI355REC_EMBED_BATCH_MAX_TOPN) {
        std::snprintf(msg, cap, "topn %d out of [1, %d] (a user batch has one round)", static_cast<int>(full->topn), MI355REC_EMBED_BATCH_MAX_TOPN);
        return true;
    }
    if (full->metric != MI355REC_EMBED_COSINE && full->metric != MI355REC_EMBED_DOT) {
        std::snprintf(msg, cap, "metric %d in an embed batch query: MI355REC_EMBED_COSINE (0) or MI355REC_EMBED_DOT (1)", static_cast<int>(full->metric));
        return true;
    }
    if (!(std::fabs(full->w_embed) <= MI355REC_EMBED_MAX_WEIGHT) || full->w_embed == 0.0f) {   // (false for NaN)
        std::snprintf(msg, cap, "embed_weight %g: finite, not 0 and at most %g in magnitude", static_cast<double>(full->w_embed),
                      static_cast<double>(MI355REC_EMBED_MAX_WEIGHT));
        return true;
    }
    if ((full->exclude_global == nullptr) != (full->exclude_offsets == nullptr)) {
        std::snprintf(msg, cap, "exclude_global and exclude_offsets: both or neither");
        return true;
    }
    if (full->exclude_offsets) {
        const int64_t* off = full->exclude_offsets;
        if (off[0] < 0) {
            std::snprintf(msg, cap, "exclude_offsets[0] is %lld: offsets are >= 0", static_cast<long long>(off[0]));
            return true;
        }
        for (int b = 0; b < full->n_users; ++b) {
            if (off[b + 1] < off[b]) {
                std::snprintf(msg, cap, "exclude_offsets decrease at user %d (%lld after %lld)", b, static_cast<long long>(off[b + 1]),
                              static_cast<long long>(off[b]));
                return true;
            }
            if (off[b + 1] - off[b] > MI355REC_EMBED_BATCH_MAX_EXCLUDE) {
                std::snprintf(msg, cap, "user %d excludes %lld ids: at most %d", b, static_cast<long long>(off[b + 1] - off[b]),
                              MI355REC_EMBED_BATCH_MAX_EXCLUDE);
                return true;
            }
        }
    }
    r->users = full->users;
    r->n_users = full->n_users;
    r->exclude = full->exclude_global;
    r->exclude_offsets = full->exclude_offsets;
    r->topn = full->topn;
    r->metric = full->metric;
    r->w_embed = full->w_embed;
    return false;
}

// The exclusion lists as the scan searches them: per user the LOCAL rows of a table of n_rows rows that starts at global
// row row_base, sorted and distinct (foreign and negative ids are dropped), one list after the other in `rows`, with
// n_users + 1 offsets.  May throw std::bad_alloc.
inline void normalise_exclusions(const BatchRequest& r, int64_t row_base, int64_t n_rows, std::vector<uint32_t>* rows, std::vector<int64_t>* offsets) {
    rows->clear();
    offsets->assign(static_cast<size_t>(r.n_users) + 1, 0);
    if (!r.exclude_offsets) return;
    for (int b = 0; b < r.n_users; ++b) {
        const size_t begin = rows->size();
        for (int64_t i = r.exclude_offsets[b]; i < r.exclude_offsets[b + 1]; ++i) {
            const int64_t id = r.exclude[i];
            if (id < row_base || id - row_base >= n_rows) continue;   // (compared before the subtraction can overflow)
            rows->push_back(static_cast<uint32_t>(id - row_base));
        }
        std::sort(rows->begin() + static_cast<std::ptrdiff_t>(begin), rows->end());
        rows->erase(std::unique(rows->begin() + static_cast<std::ptrdiff_t>(begin), rows->end()), rows->end());
        (*offsets)[static_cast<size_t>(b) + 1] = static_cast<int64_t>(rows->size());
    }
}

// User b's n sorted keys into the batch result (idx / score padded to topn, count).
inline void write_batch_result(const uint64_t* keys, int n, int topn, int b, const mi355rec_embed_batch_result_t& res) {
    mi355rec_embed_result_t one{};
    one.size = sizeof one;
    one.out_idx = res.out_idx + static_cast<int64_t>(b) * topn;
    one.out_score = res.out_score ? res.out_score + static_cast<int64_t>(b) * topn : nullptr;
    one.out_count = nullptr;
    write_result(keys, n, topn, one);
    if (res.out_count) res.out_count[b] = n;
}

}  // namespace mi355embed
