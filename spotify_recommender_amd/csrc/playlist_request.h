// playlist_request.h — ONE description of a call of the playlist family (include/mi355rec_diag.h: "PLAYLISTS", "FEATURE
// FILTERS", "WEIGHTED PLAYLISTS", "DIVERSIFIED TOP-N", "GROUP CAPS"), its outputs and its argument checks, shared by the single
// handle (engine_playlist.hip.h), the node handle (sharded.hip) and the CPU backend.  Every exported entry point of the
// family fills a Request and an Outputs and takes the one path of its handle type; neither struct is part of the C-ABI.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "filter_check.h"
#include "mi355rec_diag.h"
#include "weights_check.h"

namespace mi355playlist {

struct Request {
    const float* members = nullptr;             // k x 12 floats by value, or null with ...
    const int64_t* rows = nullptr;              // ... k rows of the handle (excluded from the results whatever their weight)
    int k = 0;
    const float* weights = nullptr;             // null (the plain mean), or k signed weights
    const int64_t* exclude = nullptr;           // n_exclude global ids, any order, duplicates allowed
    int n_exclude = 0;
    const mi355rec_filter_t* filter = nullptr;  // null, or the feature filter
    int topn = 0;
    bool diverse = false;                       // the top-`pool` re-ranked by maximal marginal relevance with `lambda`
    float lambda = 1.0f;
    int pool = 0;
    bool capped = false;                        // (diverse only) at most max_per_group picks per group ...
    int max_per_group = 0;                      // ... >= 1 then; 0 in every call that is not capped

    int scan_topn() const { return diverse ? pool : topn; }   // what the scan selects
    // The same call diversified, and (of a diversified one) capped: what the _diverse and _capped entry points add.
    Request diversified(float lambda_, int pool_) const {
        Request r = *this;
        r.diverse = true;
        r.lambda = lambda_;
        r.pool = pool_;
        return r;
    }
    // The plain call that selects a diversified one's pool: its top-`pool`.
    Request pool_call() const {
        Request r = *this;
        r.diverse = r.capped = false;
        r.topn = pool;
        return r;
    }
    Request capped_at(int max_per_group_) const {
        Request r = *this;
        r.capped = true;
        r.max_per_group = max_per_group_;
        return r;
    }
};

// The arguments every exported call of the family has, in the order the _weighted calls take them (members or rows is null;
// the levels below _weighted pass null weights / a null filter).
inline Request request(const float* members, const int64_t* rows, const float* weights, int k, const int64_t* exclude, int n_exclude,
                       const mi355rec_filter_t* filter, int topn) {
    Request r;
    r.members = members;
    r.rows = rows;
    r.k = k;
    r.weights = weights;
    r.exclude = exclude;
    r.n_exclude = n_exclude;
    r.filter = filter;
    r.topn = topn;
    return r;
}

// Where the results go.  idx is never null; every other pointer may be.
struct Outputs {
    int64_t* idx = nullptr;
    float* score = nullptr;
    float* mmr = nullptr;       // diverse only
    int* count = nullptr;
    int* pool_rows = nullptr;   // capped only: P'
};

// idx / score / mmr [from, topn) padded with -1 / 0.0f / 0.0f, and *count set.
inline void pad(const Outputs& out, int from, int topn, int count) {
    for (int i = from; i < topn; ++i) {
        out.idx[i] = -1;
        if (out.score) out.score[i] = 0.0f;
        if (out.mmr) out.mmr[i] = 0.0f;
    }
    if (out.count) *out.count = count;
}

// True when the lambda, topn, pool or cap of a diverse request cannot be used; then msg[0..cap) says why.
inline bool invalid_diverse(const Request& r, char* msg, size_t cap) {
    if (std::isnan(r.lambda) || r.lambda < 0.0f || r.lambda > 1.0f) {
        std::snprintf(msg, cap, "lambda %g out of [0, 1]", static_cast<double>(r.lambda));
        return true;
    }
    if (r.topn <= 0) {
        std::snprintf(msg, cap, "topn must be positive, got %d", r.topn);
        return true;
    }
    if (r.pool < r.topn || r.pool > MI355REC_MAX_TOPN_FAST) {
        std::snprintf(msg, cap, "pool %d out of [topn = %d, %d]", r.pool, r.topn, MI355REC_MAX_TOPN_FAST);
        return true;
    }
    if (r.capped && r.max_per_group < 1) {
        std::snprintf(msg, cap, "max_per_group must be positive, got %d", r.max_per_group);
        return true;
    }
    return false;
}

// True when the playlist part of `r` (members or rows non-null) cannot be used; then msg[0..cap) says why.  What the two
// handle types do not share: an excluded id lies in [0, exclude_end) (the single handle takes any uint32 global id, the node
// knows its catalogue), at most max_exclude of them (the node's own calls into a shard carry the members' rows as well); rows
// lie in [0, n_rows).
inline bool invalid_playlist(const Request& r, int64_t n_rows, int64_t exclude_end, int max_exclude, char* msg, size_t cap) {
    const int topn = r.scan_topn();
    if (r.k < 1 || r.k > MI355REC_MAX_PLAYLIST) {
        std::snprintf(msg, cap, "playlist of %d songs: 1 to %d are supported", r.k, MI355REC_MAX_PLAYLIST);
        return true;
    }
    if (topn <= 0 || topn > MI355REC_MAX_TOPN_FAST) {
        std::snprintf(msg, cap, "topn %d out of [1, %d] (a playlist query has one round)", topn, MI355REC_MAX_TOPN_FAST);
        return true;
    }
    if (r.n_exclude < 0 || r.n_exclude > max_exclude) {
        std::snprintf(msg, cap, "n_exclude %d out of [0, %d]", r.n_exclude, max_exclude);
        return true;
    }
    if (r.n_exclude > 0 && !r.exclude) {
        std::snprintf(msg, cap, "null exclusion list with n_exclude %d", r.n_exclude);
        return true;
    }
    for (int i = 0; i < r.n_exclude; ++i)
        if (r.exclude[i] < 0 || r.exclude[i] >= exclude_end) {
            std::snprintf(msg, cap, "excluded row %lld out of the catalogue", static_cast<long long>(r.exclude[i]));
            return true;
        }
    if (r.rows)
        for (int m = 0; m < r.k; ++m)
            if (r.rows[m] < 0 || r.rows[m] >= n_rows) {
                std::snprintf(msg, cap, "Invalid song index: %lld", static_cast<long long>(r.rows[m]));
                return true;
            }
    if (r.filter && mi355filter::invalid(r.filter, msg, cap)) return true;
    if (r.weights && mi355weights::invalid(r.weights, r.k, msg, cap)) return true;
    return false;
}

}  // namespace mi355playlist
