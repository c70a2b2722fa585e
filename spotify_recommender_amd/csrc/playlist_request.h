// playlist_request.h — ONE description of a call of the playlist family (include/mi355rec_diag.h: "PLAYLISTS", "FEATURE
// FILTERS", "WEIGHTED PLAYLISTS", "DIVERSIFIED TOP-N", "GROUP CAPS"), its outputs and its argument checks, shared by the single
// handle (engine_playlist.hip.h), the node handle (sharded.hip) and the CPU backend.  Every exported entry point of the
// family fills a Request and an Outputs and takes the one path of its handle type.  Neither struct is part of the C-ABI; the
// C-ABI's own request structs are converted to them by from_request below, one overload per struct: the playlist request
// ("PLAYLIST REQUESTS": mi355rec_playlist_query_t, with its flags) by its own body, the four 64-byte metric requests ("DISTANCE
// REQUESTS", "ANY-OF REQUESTS", "MANHATTAN REQUESTS", "JACCARD REQUESTS": the same Request with another `metric`) by ONE body, from_metric_query, over a
// MetricKind row each.  Every self-sized struct (the four requests and the ext) is read by read_sized; every kind applies the ext
// through from_ext then apply_ext.  A further metric request is a MetricKind row, an outputs_of mapping and an overload.
// The bounded request ("BOUNDED REQUESTS": mi355rec_bounded_query_t, the metric requests' 64 bytes and then `metric` and `bound`) has
// its own overload and its own refusal texts: the same Request with `bounded`, `floor_thr` and `floor_score`, and Outputs::total.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "filter_check.h"
#include "mi355rec_diag.h"
#include "weights_check.h"

namespace mi355playlist {

enum Metric { kCosine = 0, kDistance = 1, kAnyOf = 2, kManhattan = 3, kJaccard = 4 };

struct Request {
    const float* members = nullptr;             // k x 12 floats by value, or null with ...
    const int64_t* rows = nullptr;              // ... k rows of the handle (excluded from the results whatever their weight)
    int k = 0;
    const float* weights = nullptr;             // null (the plain mean), or k signed weights
    const int64_t* exclude = nullptr;           // n_exclude global ids, any order, duplicates allowed
    int n_exclude = 0;
    const mi355rec_filter_t* filter = nullptr;  // null, or the feature filter
    const int32_t* labels = nullptr;            // null (every row), or n_labels labels in [0, MI355REC_MAX_LABELS): only rows
    int n_labels = 0;                           // ... whose label is in the set are admissible ("PLAYLIST REQUESTS")
    int topn = 0;
    bool diverse = false;                       // the top-`pool` re-ranked by maximal marginal relevance with `lambda`
    float lambda = 1.0f;
    int pool = 0;
    bool capped = false;                        // (diverse only) at most max_per_group picks per group ...
    int max_per_group = 0;                      // ... >= 1 then; 0 in every call that is not capped
    bool prior = false;                         // rank by v = fl(score + fl(prior_weight p(x))), p the handle's priors ("ROW PRIORS")
    float prior_weight = 0.0f;                  // ... beta, finite, |beta| <= MI355REC_MAX_PRIOR_WEIGHT; 0.0f is the call without a prior
    int metric = kCosine;                       // kDistance ("DISTANCE REQUESTS"): rank by m(x), the mean squared distance to the
                                                // ... members, ascending; keys and scores carry -m
                                                // kAnyOf ("ANY-OF REQUESTS"): rank by v(x), the best of the members' cosines
                                                // kManhattan ("MANHATTAN REQUESTS"): rank by m(x), the mean L1 distance to the members,
                                                // ... ascending; keys and scores carry -m
                                                // kJaccard ("JACCARD REQUESTS"): rank by v(x), the mean weighted Jaccard similarity to
                                                // ... the members, descending; keys and scores carry v
    bool attribute = false;                     // (kAnyOf) the member index a(x) of every result is wanted (Outputs::member)
    bool report_distance = false;               // (kDistance, kManhattan) the score output holds sqrtf(m) (kManhattan: m, no root);
                                                // ... false: -m itself, what a node
                                                // ... handle's merge over shards compares
    const float* scales = nullptr;              // null, or 12 checked feature scales a_j ("FEATURE SCALES"): the call is the same
                                                // ... call on rows fl(a_j x_j) with members fl(a_j q_kj); the filter tests x itself
    const mi355rec_rowset_t* rowset = nullptr;  // null, or the row set ("ROW SETS", rowset.h): with rowset_only only its rows are
    bool rowset_only = false;                   // ... admissible, without it only the others
    bool listed = false;                        // "CANDIDATE LISTS" (candidates.h): only the n_candidates checked global ids of
    const int64_t* candidates = nullptr;        // ... `candidates` are admissible (any order, duplicates allowed; n_candidates == 0:
    int64_t n_candidates = 0;                   // ... no row is), beside whatever else the request asks of a row
    int64_t candidates_id_end = -1;             // >= 0: the ids are NOT checked yet: each lies in [0, this), or the request is refused
                                                // ... by the pass that reduces the list (the single handle's own entry points)
    bool score = false;                         // "CANDIDATE SCORES" (listed only): the value of EVERY listed row is wanted, in list
                                                // ... order, and nothing is selected: topn is checked and otherwise unused
    bool bounded = false;                       // "BOUNDED REQUESTS" (kCosine, kDistance): only rows whose key exceeds floor_thr MATCH;
    uint64_t floor_thr = 0;                     // ... their exact number is wanted (Outputs::total) and topn may be 0 (count only);
    float floor_score = 0.0f;                   // ... b, the score floor_thr was made from (bounded_floor): a key's score s matches iff s >= b

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
    Request with_prior(float weight) const {
        Request r = *this;
        r.prior = true;
        r.prior_weight = weight;
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
    int32_t* member = nullptr;  // "ANY-OF REQUESTS" only: a(x) of every result
    int64_t* total = nullptr;   // "BOUNDED REQUESTS" only: the number of matching rows
};

// idx / score / mmr [from, topn) padded with -1 / 0.0f / 0.0f, and *count set.
inline void pad(const Outputs& out, int from, int topn, int count) {
    for (int i = from; i < topn; ++i) {
        out.idx[i] = -1;
        if (out.score) out.score[i] = 0.0f;
        if (out.mmr) out.mmr[i] = 0.0f;
        if (out.member) out.member[i] = -1;
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
    if (r.bounded && (topn < 0 || topn > MI355REC_MAX_TOPN_FAST)) {
        std::snprintf(msg, cap, "topn %d out of [0, %d] (a bounded query has one round; 0 counts only)", topn, MI355REC_MAX_TOPN_FAST);
        return true;
    }
    if (!r.bounded && (topn <= 0 || topn > MI355REC_MAX_TOPN_FAST)) {
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
    // the label set: the messages of the label calls (engine_labels.hip.h, label_mask)
    if (r.n_labels < 0 || (r.labels && r.n_labels == 0)) {
        std::snprintf(msg, cap, "n_labels must be positive, got %d", r.n_labels);
        return true;
    }
    if (r.n_labels > 0 && !r.labels) {
        std::snprintf(msg, cap, "null label set");
        return true;
    }
    for (int i = 0; i < r.n_labels; ++i)
        if (r.labels[i] < 0 || r.labels[i] >= MI355REC_MAX_LABELS) {
            std::snprintf(msg, cap, "label %d out of [0, %d)", static_cast<int>(r.labels[i]), MI355REC_MAX_LABELS);
            return true;
        }
    if (r.prior && !(std::fabs(r.prior_weight) <= MI355REC_MAX_PRIOR_WEIGHT)) {   // (false for NaN)
        std::snprintf(msg, cap, "prior_weight %g out of [-%g, %g]", static_cast<double>(r.prior_weight),
                      static_cast<double>(MI355REC_MAX_PRIOR_WEIGHT), static_cast<double>(MI355REC_MAX_PRIOR_WEIGHT));
        return true;
    }
    return false;
}

// The first row whose prior cannot be used (not finite, or |p| > 1), or -1 ("ROW PRIORS": mi355rec_set_priors).
inline int64_t first_bad_prior(const float* priors, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(std::fabs(priors[i]) <= 1.0f)) return i;   // (false for NaN)
    return -1;
}

// The label set of a checked request as a mask: bit l of mask[l / 32] (MI355REC_MAX_LABELS / 32 words).
inline void label_bits(const Request& r, uint32_t* mask) {
    for (int w = 0; w < MI355REC_MAX_LABELS / 32; ++w) mask[w] = 0u;
    for (int i = 0; i < r.n_labels; ++i) mask[r.labels[i] >> 5] |= 1u << (r.labels[i] & 31);
}

// "DISTANCE REQUESTS": out.score[0..count) holds -m (the key's score, +0.0 for m = 0); the reported distance is sqrtf(m).
// (0.0f - s, not -s: the distance of m = 0 is +0.0f.)  "MANHATTAN REQUESTS" (metric kManhattan): m itself, there is no root.
inline void scores_to_distances(const Outputs& out, int topn, int metric = kDistance) {
    if (!out.score) return;
    for (int i = 0; i < topn && out.idx[i] >= 0; ++i) {
        const float m = 0.0f - out.score[i];
        out.score[i] = metric == kManhattan ? m : std::sqrt(m);
    }
}

// "CANDIDATE SCORES": where the values go, in list order: value[i] and (may be null) admissible[i] for candidates[i].
struct ScoreOutputs {
    float* value = nullptr;
    uint8_t* admissible = nullptr;
};

// ... the entry of a candidate that is not admissible: the quiet NaN 0x7fc00000, flag 0.
inline void score_none(const ScoreOutputs& out, int64_t i) {
    const uint32_t nan_bits = 0x7fc00000u;
    std::memcpy(&out.value[i], &nan_bits, sizeof nan_bits);
    if (out.admissible) out.admissible[i] = 0;
}

// ... and of one that is: `s` is the key's score (+0.0 for -0.0 already; -m for a distance request: sqrtf(0.0f - s) is reported).
inline void score_some(const Request& r, const ScoreOutputs& out, int64_t i, float s) {
    out.value[i] = r.report_distance ? std::sqrt(0.0f - s) : s;
    if (out.admissible) out.admissible[i] = 1;
}

// ... what the scoring calls refuse beyond the _candidates calls' own checks (r: the converted request).  True: msg says why.
inline bool invalid_score_request(const Request& r, int64_t n_candidates, const float* out_value, char* msg, size_t cap) {
    if (r.diverse) {
        std::snprintf(msg, cap, "%s in a candidate scores call: a re-ranked order has no per-row value",
                      r.capped ? "MI355REC_PQ_CAPPED" : "MI355REC_PQ_DIVERSE");
        return true;
    }
    if (n_candidates > 0 && !out_value) {
        std::snprintf(msg, cap, "candidate scores: null out_value with n_candidates %lld", static_cast<long long>(n_candidates));
        return true;
    }
    return false;
}

// The size rule of every self-sized struct of the C-ABI (its first field is `uint32_t size`): in->size says how much of the
// struct the caller knows.  It must be the end of a field (`ends`, the full size last: a struct that ends inside a field would hand
// over half a pointer); a shorter one is read as "later fields zero"; 0, or more than this library knows, is refused.  True when
// refused; then msg[0..cap) says why, naming the struct `what`.  Otherwise *full holds the struct as this library reads it.
template <class T, size_t N>
inline bool read_sized(const T* in, const char* what, const size_t (&ends)[N], T* full, char* msg, size_t cap) {
    bool known = false;
    for (size_t e : ends) known = known || in->size == e;
    if (!known) {
        std::snprintf(msg, cap, "%s of size %u: not the end of a field of the %u bytes this library reads", what,
                      static_cast<unsigned>(in->size), static_cast<unsigned>(sizeof *full));
        return true;
    }
    std::memset(full, 0, sizeof *full);
    std::memcpy(full, in, in->size);
    return false;
}

// The C-ABI's request (include/mi355rec_diag.h, "PLAYLIST REQUESTS") as the Request and Outputs every layer below takes, read by
// read_sized' rule.  True when the structs cannot be used; then msg[0..cap) says why.
inline bool from_query(const mi355rec_playlist_query_t* q, const mi355rec_playlist_result_t* res, mi355rec_playlist_query_t* full,
                       Request* r, Outputs* out, char* msg, size_t cap) {
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(mi355rec_playlist_query_t, flags),          offsetof(mi355rec_playlist_query_t, members),
                                  offsetof(mi355rec_playlist_query_t, rows),           offsetof(mi355rec_playlist_query_t, weights),
                                  offsetof(mi355rec_playlist_query_t, exclude_global), offsetof(mi355rec_playlist_query_t, filter),
                                  offsetof(mi355rec_playlist_query_t, labels),         offsetof(mi355rec_playlist_query_t, k),
                                  offsetof(mi355rec_playlist_query_t, n_exclude),      offsetof(mi355rec_playlist_query_t, n_labels),
                                  offsetof(mi355rec_playlist_query_t, topn),           offsetof(mi355rec_playlist_query_t, lambda),
                                  offsetof(mi355rec_playlist_query_t, pool),           offsetof(mi355rec_playlist_query_t, max_per_group),
                                  offsetof(mi355rec_playlist_query_t, prior_weight), sizeof(mi355rec_playlist_query_t)};
    static_assert(offsetof(mi355rec_playlist_query_t, prior_weight) == offsetof(mi355rec_playlist_query_t, max_per_group) + sizeof(int32_t) &&
                      offsetof(mi355rec_playlist_query_t, prior_weight) == 84 && sizeof(mi355rec_playlist_query_t) == 88,
                  "prior_weight fills the tail padding: the struct ends where the field ends");
    if (read_sized(q, "playlist query", ends, full, msg, cap)) return true;
    if (full->flags & ~static_cast<uint32_t>(MI355REC_PQ_DIVERSE | MI355REC_PQ_CAPPED | MI355REC_PQ_PRIOR)) {
        std::snprintf(msg, cap, "unknown flags 0x%x in a playlist query", static_cast<unsigned>(full->flags));
        return true;
    }
    if ((full->flags & MI355REC_PQ_CAPPED) && !(full->flags & MI355REC_PQ_DIVERSE)) {
        std::snprintf(msg, cap, "MI355REC_PQ_CAPPED needs MI355REC_PQ_DIVERSE");
        return true;
    }
    // prior_weight lies in what was tail padding: an older caller's bytes there are garbage, so it is read only with the flag,
    // and only from a struct whose size covers it
    if ((full->flags & MI355REC_PQ_PRIOR) && q->size < offsetof(mi355rec_playlist_query_t, prior_weight) + sizeof(float)) {
        std::snprintf(msg, cap, "MI355REC_PQ_PRIOR in a playlist query of size %u: prior_weight ends at %u", static_cast<unsigned>(q->size),
                      static_cast<unsigned>(offsetof(mi355rec_playlist_query_t, prior_weight) + sizeof(float)));
        return true;
    }
    if (full->members && full->rows) {
        std::snprintf(msg, cap, "members by value and by row in one playlist query");
        return true;
    }
    *r = request(full->members, full->rows, full->weights, full->k, full->exclude_global, full->n_exclude, full->filter, full->topn);
    r->labels = full->labels;
    r->n_labels = full->n_labels;
    if (full->flags & MI355REC_PQ_DIVERSE) *r = r->diversified(full->lambda, full->pool);
    if (full->flags & MI355REC_PQ_CAPPED) *r = r->capped_at(full->max_per_group);
    if (full->flags & MI355REC_PQ_PRIOR) *r = r->with_prior(full->prior_weight);
    *out = {res->out_idx, res->out_score, r->diverse ? res->out_mmr : nullptr, res->out_count, res->out_pool_rows};
    return false;
}

// "FEATURE SCALES": true when the 12 scales cannot be used (each finite, 0 <= a_j <= MI355REC_MAX_FEATURE_SCALE, -0.0f is 0; at
// least one > 0); then msg[0..cap) names the feature and its value.
inline bool invalid_scales(const float* a, char* msg, size_t cap) {
    bool any = false;
    for (int j = 0; j < MI355REC_DIM; ++j) {
        if (!(a[j] >= 0.0f && a[j] <= MI355REC_MAX_FEATURE_SCALE)) {   // (false for NaN)
            std::snprintf(msg, cap, "feature scale %d is %g: a scale is finite and in [0, %g]", j, static_cast<double>(a[j]),
                          static_cast<double>(MI355REC_MAX_FEATURE_SCALE));
            return true;
        }
        any = any || a[j] > 0.0f;
    }
    if (!any) {
        std::snprintf(msg, cap, "every feature scale is 0: at least one must be positive");
        return true;
    }
    return false;
}

// The scales of a checked request as the launch takes them: null when there are none or every one is 1.0f (fl(1 x) = x: the
// unscaled call bit for bit, so it takes the unscaled launch).
inline const float* effective_scales(const float* a) {
    if (!a) return nullptr;
    for (int j = 0; j < MI355REC_DIM; ++j)
        if (a[j] != 1.0f) return a;
    return nullptr;
}

// "ROW SETS": the per-request extras (mi355rec_request_ext_t) as this library reads them, by read_sized' rule.  A null ext is the
// ext with every field zero.  True when it cannot be used; then msg says why.
inline bool from_ext(const mi355rec_request_ext_t* ext, mi355rec_request_ext_t* full, char* msg, size_t cap) {
    if (!ext) {
        std::memset(full, 0, sizeof *full);
        return false;
    }
    static const size_t ends[] = {offsetof(mi355rec_request_ext_t, rowset_mode), offsetof(mi355rec_request_ext_t, feature_scales),
                                  offsetof(mi355rec_request_ext_t, rowset), sizeof(mi355rec_request_ext_t)};
    static_assert(sizeof(mi355rec_request_ext_t) == 24 && offsetof(mi355rec_request_ext_t, rowset) == 16, "the struct ends where its last field ends");
    if (read_sized(ext, "request ext", ends, full, msg, cap)) return true;
    if (full->rowset && full->rowset_mode != MI355REC_ROWSET_EXCLUDE && full->rowset_mode != MI355REC_ROWSET_ONLY) {
        std::snprintf(msg, cap, "rowset_mode %u: MI355REC_ROWSET_EXCLUDE (0) or MI355REC_ROWSET_ONLY (1)", static_cast<unsigned>(full->rowset_mode));
        return true;
    }
    return false;
}

// The extras of a checked ext into the Request (the scales checked here: invalid_scales' messages).
inline bool apply_ext(const mi355rec_request_ext_t& ext, Request* r, char* msg, size_t cap) {
    if (ext.feature_scales) {
        if (invalid_scales(ext.feature_scales, msg, cap)) return true;
        r->scales = effective_scales(ext.feature_scales);
    }
    r->rowset = ext.rowset;
    r->rowset_only = ext.rowset && ext.rowset_mode == MI355REC_ROWSET_ONLY;
    return false;
}

// The playlist request with its extras, as every entry point that takes the struct converts it (the _scaled ones pass an ext that
// holds their scales): every check of from_query first (its messages), then the ext's own; with scales, flags must be 0 and the
// scales usable.  A null ext, or one whose pointers are null, is from_query itself.
inline bool from_request(const mi355rec_playlist_query_t* q, const mi355rec_request_ext_t* ext, const mi355rec_playlist_result_t* res,
                         mi355rec_playlist_query_t* full, Request* r, Outputs* out, char* msg, size_t cap) {
    if (from_query(q, res, full, r, out, msg, cap)) return true;
    mi355rec_request_ext_t x;
    if (from_ext(ext, &x, msg, cap)) return true;
    if (x.feature_scales) {
        static const struct { uint32_t bit; const char* name; } refused[] = {{MI355REC_PQ_DIVERSE, "MI355REC_PQ_DIVERSE"},
                                                                             {MI355REC_PQ_CAPPED, "MI355REC_PQ_CAPPED"},
                                                                             {MI355REC_PQ_PRIOR, "MI355REC_PQ_PRIOR"}};
        for (const auto& f : refused)
            if (full->flags & f.bit) {
                std::snprintf(msg, cap, "%s with feature scales: flags must be 0 (diversified and capped calls and priors are not served)", f.name);
                return true;
            }
    }
    return apply_ext(x, r, msg, cap);
}

// The ext a _scaled entry point passes on: its scales and nothing else.
inline mi355rec_request_ext_t scales_only_ext(const float* scales) {
    mi355rec_request_ext_t x;
    std::memset(&x, 0, sizeof x);
    x.size = static_cast<uint32_t>(sizeof x);
    x.feature_scales = scales;
    return x;
}

// The four 64-byte metric requests of the C-ABI (include/mi355rec_diag.h: "DISTANCE REQUESTS", "ANY-OF REQUESTS", "MANHATTAN
// REQUESTS", "JACCARD REQUESTS") are one layout under four names; what tells them apart is a row of this table ...
struct MetricKind {
    const char* noun;        // the struct as the messages name it, with its article
    int metric;
    bool report_distance;    // the score output holds the distance (Request::report_distance)
    const char* no_scales;   // null: feature scales are served; or the text that refuses them
};
constexpr MetricKind kDistanceQuery = {"a distance query", kDistance, true, nullptr};
constexpr MetricKind kAnyOfQuery = {"an any-of query", kAnyOf, false, "any-of requests take no feature scales"};
constexpr MetricKind kManhattanQuery = {"a manhattan query", kManhattan, true, "manhattan requests take no feature scales"};
constexpr MetricKind kJaccardQuery = {"a jaccard query", kJaccard, false, "jaccard requests take no feature scales"};

// ... and where its result struct's pointers go (any-of's carries out_member: the attribution is wanted when it is given).
inline Outputs outputs_of(const mi355rec_distance_result_t& res) { return {res.out_idx, res.out_distance, nullptr, res.out_count, nullptr}; }
inline Outputs outputs_of(const mi355rec_manhattan_result_t& res) { return {res.out_idx, res.out_distance, nullptr, res.out_count, nullptr}; }
inline Outputs outputs_of(const mi355rec_jaccard_result_t& res) { return {res.out_idx, res.out_similarity, nullptr, res.out_count, nullptr}; }
inline Outputs outputs_of(const mi355rec_anyof_result_t& res) {
    return {res.out_idx, res.out_score, nullptr, res.out_count, nullptr, res.out_member};
}

// A metric request with its extras as the same Request (metric = kind.metric) and Outputs: read_sized' rule, flags must be 0,
// members by value or by row, then the ext (a null one, or one whose pointers are null, adds nothing).  True when the structs
// cannot be used; then msg[0..cap) says why.
template <class Query, class Result>
inline bool from_metric_query(const MetricKind& kind, const Query* q, const mi355rec_request_ext_t* ext, const Result* res, Query* full,
                              Request* r, Outputs* out, char* msg, size_t cap) {
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Query, flags),  offsetof(Query, members), offsetof(Query, rows), offsetof(Query, exclude_global),
                                  offsetof(Query, filter), offsetof(Query, labels),  offsetof(Query, k),    offsetof(Query, n_exclude),
                                  offsetof(Query, n_labels), offsetof(Query, topn),  sizeof(Query)};
    static_assert(sizeof(Query) == offsetof(Query, topn) + sizeof(int32_t) && sizeof(Query) == 64,
                  "no tail padding: the struct ends where its last field ends");
    const char* bare = std::strchr(kind.noun, ' ') + 1;   // the noun without its article
    if (read_sized(q, bare, ends, full, msg, cap)) return true;
    if (full->flags != 0u) {
        std::snprintf(msg, cap, "flags 0x%x in %s: must be 0 (weights, diversified and capped calls and priors are not served)",
                      static_cast<unsigned>(full->flags), kind.noun);
        return true;
    }
    if (full->members && full->rows) {
        std::snprintf(msg, cap, "members by value and by row in one %s", bare);
        return true;
    }
    if (!full->members && !full->rows) {
        std::snprintf(msg, cap, "%s needs members by value or by row", kind.noun);
        return true;
    }
    *r = request(full->members, full->rows, nullptr, full->k, full->exclude_global, full->n_exclude, full->filter, full->topn);
    r->labels = full->labels;
    r->n_labels = full->n_labels;
    r->metric = kind.metric;
    r->report_distance = kind.report_distance;
    *out = outputs_of(*res);
    r->attribute = out->member != nullptr;
    mi355rec_request_ext_t x;
    if (from_ext(ext, &x, msg, cap)) return true;
    if (x.feature_scales && kind.no_scales) {
        std::snprintf(msg, cap, "%s", kind.no_scales);
        return true;
    }
    return apply_ext(x, r, msg, cap);
}

inline bool from_request(const mi355rec_distance_query_t* q, const mi355rec_request_ext_t* ext, const mi355rec_distance_result_t* res,
                         mi355rec_distance_query_t* full, Request* r, Outputs* out, char* msg, size_t cap) {
    return from_metric_query(kDistanceQuery, q, ext, res, full, r, out, msg, cap);
}
inline bool from_request(const mi355rec_anyof_query_t* q, const mi355rec_request_ext_t* ext, const mi355rec_anyof_result_t* res,
                         mi355rec_anyof_query_t* full, Request* r, Outputs* out, char* msg, size_t cap) {
    return from_metric_query(kAnyOfQuery, q, ext, res, full, r, out, msg, cap);
}
inline bool from_request(const mi355rec_manhattan_query_t* q, const mi355rec_request_ext_t* ext, const mi355rec_manhattan_result_t* res,
                         mi355rec_manhattan_query_t* full, Request* r, Outputs* out, char* msg, size_t cap) {
    return from_metric_query(kManhattanQuery, q, ext, res, full, r, out, msg, cap);
}
inline bool from_request(const mi355rec_jaccard_query_t* q, const mi355rec_request_ext_t* ext, const mi355rec_jaccard_result_t* res,
                         mi355rec_jaccard_query_t* full, Request* r, Outputs* out, char* msg, size_t cap) {
    return from_metric_query(kJaccardQuery, q, ext, res, full, r, out, msg, cap);
}

// "BOUNDED REQUESTS": the ordered image of a score as keys carry it (core.hip.h, score_to_ordered: -0.0 and +0.0 share one).
inline uint32_t ordered_image(float s) {
    s = s + 0.0f;
    uint32_t u;
    std::memcpy(&u, &s, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ... the floor of a bounded request: a key matches iff key > floor_thr, that is iff its score's image is at least b's (the row
// half of a key is never negative).  b is finite, so its image is neither 0 nor ~0.
inline uint64_t bounded_floor(float b) { return (static_cast<uint64_t>(ordered_image(b)) << 32) - 1ull; }

// ... does a result whose key carries the score s match the floor made from b?
inline bool bounded_match(float s, float b) { return ordered_image(s) >= ordered_image(b); }

// ... the Euclidean metric's b = -m_max for a checked radius (finite, >= 0): m_max is the largest float with sqrtf(m_max) <= radius,
// found from fl(radius^2) by nextafterf steps (sqrtf is correctly rounded and monotone; the steps are a handful at most).
inline float bounded_radius_floor(float radius) {
    float m = radius * radius;
    const float top = 3.4028234663852886e38f;   // FLT_MAX: m_max is finite (a row whose m is not finite never matches)
    if (!(m <= top)) m = top;
    while (m > 0.0f && std::sqrt(m) > radius) m = std::nextafter(m, 0.0f);
    while (m < top && std::sqrt(std::nextafter(m, top)) <= radius) m = std::nextafter(m, top);
    return 0.0f - m;
}

// ... the bounded request with its extras as the same Request (metric kCosine or kDistance, bounded, floor_thr) and Outputs: read_sized'
// rule, flags must be 0, members by value or by row, the metric and the bound, then the ext.  The refusal texts are this struct's
// own.  True when the structs cannot be used; then msg[0..cap) says why.
inline bool from_request(const mi355rec_bounded_query_t* q, const mi355rec_request_ext_t* ext, const mi355rec_bounded_result_t* res,
                         mi355rec_bounded_query_t* full, Request* r, Outputs* out, char* msg, size_t cap) {
    using Query = mi355rec_bounded_query_t;
    if (!q || !res) {
        std::snprintf(msg, cap, "null argument");
        return true;
    }
    static const size_t ends[] = {offsetof(Query, flags),  offsetof(Query, members), offsetof(Query, rows), offsetof(Query, exclude_global),
                                  offsetof(Query, filter), offsetof(Query, labels),  offsetof(Query, k),    offsetof(Query, n_exclude),
                                  offsetof(Query, n_labels), offsetof(Query, topn),  offsetof(Query, metric), offsetof(Query, bound),
                                  sizeof(Query)};
    static_assert(sizeof(Query) == offsetof(Query, bound) + sizeof(float) && sizeof(Query) == 72 && offsetof(Query, metric) == 64,
                  "the distance query's 64 bytes, then metric and bound; no tail padding");
    if (read_sized(q, "bounded query", ends, full, msg, cap)) return true;
    if (full->flags != 0u) {
        std::snprintf(msg, cap, "flags 0x%x in a bounded query: must be 0 (weights, diversified and capped calls and priors are not served)",
                      static_cast<unsigned>(full->flags));
        return true;
    }
    if (full->members && full->rows) {
        std::snprintf(msg, cap, "members by value and by row in one bounded query");
        return true;
    }
    if (!full->members && !full->rows) {
        std::snprintf(msg, cap, "a bounded query needs members by value or by row");
        return true;
    }
    if (full->metric != MI355REC_BOUNDED_COSINE && full->metric != MI355REC_BOUNDED_EUCLIDEAN) {
        std::snprintf(msg, cap, "metric %d in a bounded query: MI355REC_BOUNDED_COSINE (0) or MI355REC_BOUNDED_EUCLIDEAN (1)",
                      static_cast<int>(full->metric));
        return true;
    }
    const bool euclid = full->metric == MI355REC_BOUNDED_EUCLIDEAN;
    if (!std::isfinite(full->bound)) {
        std::snprintf(msg, cap, "bound %g in a bounded query: a %s is finite", static_cast<double>(full->bound), euclid ? "radius" : "floor");
        return true;
    }
    if (euclid && full->bound < 0.0f) {
        std::snprintf(msg, cap, "radius %g in a bounded query: a radius is >= 0", static_cast<double>(full->bound));
        return true;
    }
    if (!res->out_total) {
        std::snprintf(msg, cap, "null out_total in a bounded result");
        return true;
    }
    if (full->topn > 0 && !res->out_idx) {
        std::snprintf(msg, cap, "null out_idx in a bounded result with topn %d", static_cast<int>(full->topn));
        return true;
    }
    *r = request(full->members, full->rows, nullptr, full->k, full->exclude_global, full->n_exclude, full->filter, full->topn);
    r->labels = full->labels;
    r->n_labels = full->n_labels;
    r->metric = euclid ? kDistance : kCosine;
    r->report_distance = euclid;
    r->bounded = true;
    r->floor_score = euclid ? bounded_radius_floor(full->bound) : full->bound;
    r->floor_thr = bounded_floor(r->floor_score);
    *out = {res->out_idx, res->out_score, nullptr, res->out_count, nullptr, nullptr, res->out_total};
    mi355rec_request_ext_t x;
    if (from_ext(ext, &x, msg, cap)) return true;
    if (x.feature_scales) {
        std::snprintf(msg, cap, "bounded requests take no feature scales");
        return true;
    }
    return apply_ext(x, r, msg, cap);
}

// ... the host's cut of `n` results in key order at the floor: how many of the leading ones match (scores as the keys carry them:
// -m for the Euclidean metric, before scores_to_distances).
inline int bounded_cut(const Request& r, const int64_t* idx, const float* score, int n) {
    int c = 0;
    while (c < n && idx[c] >= 0 && bounded_match(score[c], r.floor_score)) ++c;
    return c;
}

// "CANDIDATE LISTS": the list an entry point was handed beside its request, if it takes one (given; {} is "no list").
struct CandidateList {
    bool given = false;
    const int64_t* ids = nullptr;
    int64_t n = 0;
};

}  // namespace mi355playlist
