// cpu_backend.cpp — see cpu_backend.h.  Own code; arithmetic contract: Recommender.cu:256-273, selection: :293-315.
#include "cpu_backend.h"

#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <vector>

namespace mi355cpu {

namespace {

constexpr int kDim = 12;   // Song.h:12 FEATURE_COUNT

// Order-preserving image of a score (larger image = larger score; -0.0f and +0.0f share one), and the packed
// candidate key of include/mi355rec.h: image << 32 | ~row, so that a larger key is the better candidate in the
// canonical order (score descending, then row ascending).  Must agree with mi355rec_pack_key (tests compare).
inline uint32_t ordered(float s) {
    s = s + 0.0f;
    uint32_t u;
    std::memcpy(&u, &s, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

inline float unordered(uint32_t o) {
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float s;
    std::memcpy(&s, &u, sizeof s);
    return s;
}

// CPUs the process may use by its cgroup quota (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us), rounded up;
// 0 = no quota (or not readable).  sched affinity is already in omp_get_max_threads().
int cpu_quota() {
    long long quota = -1, period = 0;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
        std::fclose(f);
    } else {
        if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
            if (std::fscanf(g, "%lld", &quota) != 1) quota = -1;
            std::fclose(g);
        }
        if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (std::fscanf(g, "%lld", &period) != 1) period = 0;
            std::fclose(g);
        }
    }
    if (quota <= 0 || period <= 0) return 0;
    return static_cast<int>((quota + period - 1) / period);
}

inline uint64_t pack(float s, uint32_t row) { return (static_cast<uint64_t>(ordered(s)) << 32) | static_cast<uint32_t>(~row); }

inline float query_norm(const float* q) {   // Recommender.cu:259-261
    float qn = 0.0f;
    for (int j = 0; j < kDim; ++j) qn += q[j] * q[j];
    return std::sqrt(qn);
}

inline float score(const float* q, float qn, const float* f) {   // Recommender.cu:262-272, one row
    float dot = 0.0f;
    float norm = 0.0f;
    for (int j = 0; j < kDim; ++j) {
        dot += q[j] * f[j];
        norm += f[j] * f[j];
    }
    norm = std::sqrt(norm) * qn;
    if (norm > 1e-8f) return std::max(-1.0f, std::min(1.0f, dot / norm));
    return 0.0f;
}

// Keeps the best `cap` keys it has been shown in a caller-owned buffer of 2 * cap keys, cut back by selection when
// full.  It never allocates: it is used inside an OpenMP region, which no exception may leave.
struct Best {
    uint64_t* keys = nullptr;
    size_t size = 0;
    size_t cap = 0;
    uint64_t floor = 0;   // a key must beat this to be worth keeping (rises at every cut)
    inline void offer(uint64_t k) {
        if (k <= floor) return;
        keys[size++] = k;
        if (size >= 2 * cap) cut();
    }
    void cut() {
        if (size <= cap) return;
        std::nth_element(keys, keys + (cap - 1), keys + size, std::greater<uint64_t>());
        size = cap;
        floor = keys[cap - 1] - 1;   // keys are unique (they carry the row): the cap-th best stays, nothing below it can matter
    }
};

}  // namespace

struct Catalogue {
    std::vector<float> feats;
    int64_t n = 0;
    int threads = 1;
};

Catalogue* create(const float* feats_rowmajor, int64_t n, int threads) {
    if (n < 0 || (n > 0 && !feats_rowmajor)) return nullptr;
    Catalogue* c = nullptr;
    try {   // (called from behind a C-ABI: no exception may leave)
        c = new Catalogue();
        c->n = n;
        c->feats.assign(feats_rowmajor, feats_rowmajor + static_cast<size_t>(n) * kDim);
    } catch (const std::bad_alloc&) {
        delete c;
        return nullptr;
    }
    int t = threads > 0 ? threads : omp_get_max_threads();
    if (threads <= 0) {   // no more threads than the process may really run (a cgroup quota throttles the rest)
        const int quota = cpu_quota();
        if (quota > 0 && t > quota) t = quota;
    }
    if (t < 1) t = 1;
    // a thread per ~8 k rows at most (~0.1 ms of rows: below that the fork costs more than the rows).  Measured on an
    // 8-vCPU host at 114 000 rows x top-10, the team being exactly the threads with rows (num_threads below): 1 040
    // queries/s on 2 threads, 2 970 on 4, 4 340 on 8.  (Round 4 allowed a thread per 64 k rows: with the process's whole
    // default team forked per call the idle threads' spinning made more threads look worse than they are.)
    const int64_t useful = n / 8192 + 1;
    if (t > useful) t = static_cast<int>(useful);
    c->threads = t;
    return c;
}

void destroy(Catalogue* c) { delete c; }
int64_t rows(const Catalogue* c) { return c->n; }
int threads(const Catalogue* c) { return c->threads; }
const float* row(const Catalogue* c, int64_t r) { return c->feats.data() + static_cast<size_t>(r) * kDim; }

// The team of a call is exactly the threads that have rows to score (c->threads: bounded by the cgroup quota and by one
// thread per ~64 k rows).  Without the clause every call forks the process's whole default team; the threads without
// work then spin at the join barrier — in a CPU-quota container they burn the quota the workers need.
void scores(const Catalogue* c, const float* q12, float* out_n) {
    const float qn = query_norm(q12);
    const float* f = c->feats.data();
    const int64_t n = c->n;
#pragma omp parallel for schedule(static) num_threads(c->threads)
    for (int64_t i = 0; i < n; ++i) out_n[i] = score(q12, qn, f + i * kDim);
}

namespace {
// The rows a filtered query may return: label[row] is in the set (bit l of mask[l / 32]); null = every row.
struct LabelFilter {
    const int32_t* label;
    const uint32_t* mask;
    inline bool keeps(int64_t i) const {
        const int32_t l = label[i];
        return l >= 0 && ((mask[l >> 5] >> (l & 31)) & 1u);
    }
};

int topn_impl(const Catalogue* c, const float* q12, int64_t exclude, int topn, int64_t* out_idx, float* out_score,
              const LabelFilter* filter);
}  // namespace

int topn(const Catalogue* c, const float* q12, int64_t exclude, int topn, int64_t* out_idx, float* out_score) {
    return topn_impl(c, q12, exclude, topn, out_idx, out_score, nullptr);
}

namespace {
int topn_impl(const Catalogue* c, const float* q12, int64_t exclude, int topn, int64_t* out_idx, float* out_score,
              const LabelFilter* filter) {
    if (topn <= 0 || c->n <= 0) return 0;
    const float qn = query_norm(q12);
    const float* f = c->feats.data();
    const int64_t n = c->n;
    const size_t cap = static_cast<size_t>(static_cast<int64_t>(topn) < n ? topn : n);
    // The rows go to `parts` threads in contiguous blocks.  Everything the region needs is allocated HERE, before it (a
    // std::bad_alloc from these lines reaches the caller's try / catch; one thrown inside the region would be
    // std::terminate behind the C-ABI): one flat pool, 2 * cap keys per part, and the parts' bookkeeping.
    const int parts = c->threads;
    std::vector<uint64_t> pool(static_cast<size_t>(parts) * 2 * cap);
    std::vector<Best> per_part(static_cast<size_t>(parts));
    for (int p = 0; p < parts; ++p) {
        per_part[static_cast<size_t>(p)].keys = pool.data() + static_cast<size_t>(p) * 2 * cap;
        per_part[static_cast<size_t>(p)].cap = cap;
    }
#pragma omp parallel num_threads(parts)
    {
        const int team = omp_get_num_threads();   // (may be smaller than asked for: nested regions, OMP_THREAD_LIMIT)
        const int use = parts < team ? parts : team;
        const int t = omp_get_thread_num();
        if (t < use) {
            // (fewer threads than parts: the last thread takes the remaining parts as well)
            const int p0 = t, p1 = (t == use - 1) ? parts : t + 1;
            for (int p = p0; p < p1; ++p) {
                Best& mine = per_part[static_cast<size_t>(p)];
                const int64_t lo = n * p / parts, hi = n * (p + 1) / parts;
                if (filter) {   // (the label test only where a set was given: the unfiltered loop is unchanged)
                    for (int64_t i = lo; i < hi; ++i) {
                        if (i == exclude || !filter->keeps(i)) continue;
                        mine.offer(pack(score(q12, qn, f + i * kDim), static_cast<uint32_t>(i)));
                    }
                } else {
                    for (int64_t i = lo; i < hi; ++i) {
                        if (i == exclude) continue;   // by index, not by score (Recommender.cu:296)
                        mine.offer(pack(score(q12, qn, f + i * kDim), static_cast<uint32_t>(i)));
                    }
                }
                mine.cut();   // at most cap keys per part from here on
            }
        }
    }
    // the parts' survivors, compacted to the front of the pool (part p's keys start at or behind where they go) and cut
    size_t total = 0;
    for (const Best& b : per_part) {
        std::memmove(pool.data() + total, b.keys, b.size * sizeof(uint64_t));
        total += b.size;
    }
    const size_t count = total < cap ? total : cap;
    std::partial_sort(pool.begin(), pool.begin() + count, pool.begin() + total, std::greater<uint64_t>());
    for (size_t i = 0; i < count; ++i) {
        out_idx[i] = static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(pool[i])));
        if (out_score) out_score[i] = unordered(static_cast<uint32_t>(pool[i] >> 32));
    }
    return static_cast<int>(count);
}
}  // namespace

}  // namespace mi355cpu

// ---- the handle: synchronous calls + the ticketed stream ----------------------------------------------------------
#include <chrono>

#include "candidates.h"
#include "mi355rec_diag.h"
#include "rowset.h"

namespace mi355cpu {

namespace {
constexpr int kDepth = 4;        // windows whose results are kept (the GPU path's ring, csrc/sharded.hip kStreamDepth)
constexpr int kMaxWindow = 64;

int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

struct Node {
    Catalogue* cat = nullptr;
    int window = 16;
    int s_topn = 0;                       // topn of the stream's current geometry (0: no query yet)
    int64_t next_ticket = 0;
    struct Win {
        int64_t abs = -1;
        int count = 0;
    } win[kDepth];
    std::vector<int64_t> idx;             // [kDepth][window][s_topn]
    std::vector<float> score;
    std::vector<int> counts;              // [kDepth][window]
    int64_t st_queries = 0, st_windows = 0, st_ns = 0;
    std::vector<int32_t> labels;          // mi355rec_sharded_set_labels: one per row, -1 = unlabelled (empty: none set)
    bool has_labels = false;
    std::vector<int32_t> groups;          // mi355rec_sharded_set_groups: one per row, -1 = ungrouped
    bool has_groups = false;
    std::vector<float> priors;            // mi355rec_sharded_set_priors: one per row
    bool has_priors = false;
};

Node* node_create(const float* feats_rowmajor, int64_t n) {
    Catalogue* c = create(feats_rowmajor, n, 0);
    if (!c) return nullptr;
    Node* h = new (std::nothrow) Node();
    if (!h) {
        destroy(c);
        return nullptr;
    }
    h->cat = c;
    return h;
}

void node_destroy(Node* h) {
    if (!h) return;
    destroy(h->cat);
    delete h;
}

const Catalogue* node_catalogue(const Node* h) { return h->cat; }

int node_query(Node* h, const float* q12, int64_t exclude, int topn_asked, int64_t* out_idx, float* out_score, int* out_count,
               const char** why) {
    if (topn_asked <= 0) {
        *why = "topn must be positive";
        return MI355REC_ERR_INVALID_ARG;
    }
    int c = 0;
    try {
        c = topn(h->cat, q12, exclude, topn_asked, out_idx, out_score);
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    mi355playlist::pad({out_idx, out_score, nullptr, out_count, nullptr}, c, topn_asked, c);   // the C-ABI pads with -1 / 0
    return MI355REC_OK;
}

namespace {
// One per-row attribute of the node: null clears it; otherwise the count must be the catalogue's rows and no value may be
// bad (bad_value(v): what is wrong with v, or null); assign gives the strong guarantee, so the previous values stay on failure.
template <class T, class BadValue>
int node_set_side(Node* h, std::vector<T>& dst, bool& has, const T* src, int64_t n, const char* bad_count, BadValue bad_value,
                  const char** why) {
    if (!src) {
        dst.clear();
        has = false;
        return MI355REC_OK;
    }
    if (n != rows(h->cat)) {
        *why = bad_count;
        return MI355REC_ERR_INVALID_ARG;
    }
    for (int64_t i = 0; i < n; ++i)
        if (const char* bad = bad_value(src[i])) {
            *why = bad;
            return MI355REC_ERR_INVALID_ARG;
        }
    try {
        dst.assign(src, src + n);
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    has = true;
    return MI355REC_OK;
}
}  // namespace

int node_set_labels(Node* h, const int32_t* labels, int64_t n, const char** why) {
    return node_set_side(h, h->labels, h->has_labels, labels, n, "the label count must equal the catalogue's rows",
                         [](int32_t l) { return l < -1 || l >= MI355REC_MAX_LABELS ? "a label is out of [-1, MI355REC_MAX_LABELS)" : nullptr; }, why);
}

int node_set_groups(Node* h, const int32_t* groups, int64_t n, const char** why) {
    return node_set_side(h, h->groups, h->has_groups, groups, n, "the group count must equal the catalogue's rows",
                         [](int32_t g) { return g < -1 ? "a group id is >= 0, or -1 for no group" : nullptr; }, why);
}

// (the node handle has checked the values: mi355rec_sharded_set_priors)
int node_set_priors(Node* h, const float* priors, int64_t n, const char** why) {
    return node_set_side(h, h->priors, h->has_priors, priors, n, "the prior count must equal the catalogue's rows",
                         [](float) { return static_cast<const char*>(nullptr); }, why);
}

int node_update_rows(Node* h, const int64_t* rows, int64_t count, const float* feats, const char** why) {
    if (count < 0 || (count > 0 && (!rows || !feats))) {
        *why = "null rows / negative count";
        return MI355REC_ERR_INVALID_ARG;
    }
    float* dst = h->cat->feats.data();
    for (int64_t i = 0; i < count; ++i)
        std::memcpy(dst + static_cast<size_t>(rows[i]) * kDim, feats + static_cast<size_t>(i) * kDim, sizeof(float) * kDim);
    return MI355REC_OK;
}

int node_query_labels(Node* h, const float* q12, int64_t exclude, const int32_t* set, int n_set, int topn_asked,
                      int64_t* out_idx, float* out_score, int* out_count, const char** why) {
    if (topn_asked <= 0) {
        *why = "topn must be positive";
        return MI355REC_ERR_INVALID_ARG;
    }
    if (n_set <= 0 || !set) {
        *why = "n_labels must be positive";
        return MI355REC_ERR_INVALID_ARG;
    }
    uint32_t mask[MI355REC_MAX_LABELS / 32] = {0};
    for (int i = 0; i < n_set; ++i) {
        if (set[i] < 0 || set[i] >= MI355REC_MAX_LABELS) {
            *why = "a label of the set is out of [0, MI355REC_MAX_LABELS)";
            return MI355REC_ERR_INVALID_ARG;
        }
        mask[set[i] >> 5] |= 1u << (set[i] & 31);
    }
    if (!h->has_labels) {
        *why = "this handle has no labels (mi355rec_sharded_set_labels)";
        return MI355REC_ERR_INVALID_ARG;
    }
    const LabelFilter filter{h->labels.data(), mask};
    int c = 0;
    try {
        c = topn_impl(h->cat, q12, exclude, topn_asked, out_idx, out_score, &filter);
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    mi355playlist::pad({out_idx, out_score, nullptr, out_count, nullptr}, c, topn_asked, c);
    return MI355REC_OK;
}

// "ANY-OF REQUESTS": v(x) = c_0, a = 0; for k = 1 .. K-1: if (c_k > v) { v = c_k; a = k; } — an IEEE compare, so -0.0 does not beat
// +0.0 and a is the smallest member index that attains the maximum.  c_k is score() above: the single query's chain.
static inline float anyof_best(const float* members, const float* qn, int k, const float* x, int* a) {
    float v = score(members, qn[0], x);
    *a = 0;
    for (int m = 1; m < k; ++m) {
        const float c = score(members + m * kDim, qn[m], x);
        if (c > v) {
            v = c;
            *a = m;
        }
    }
    return v;
}

// The key of every row of the catalogue under the request, 0 for a row that is not admissible (keys[i]: row i), and how many are:
// what node_query_mean selects from and node_score_rows reads.
static int mean_keys(Node* h, const mi355playlist::Request& r, std::vector<uint64_t>& keys, int64_t* admissible, const char** why) {
    const float* members = r.members;
    const float* weights = r.weights;
    const mi355rec_filter_t* filter = r.filter;
    const int k = r.k;
    if (r.n_labels > 0 && !h->has_labels) {   // "PLAYLIST REQUESTS": a label set needs labels
        *why = "this handle has no labels (mi355rec_sharded_set_labels)";
        return MI355REC_ERR_INVALID_ARG;
    }
    if (r.prior && !h->has_priors) {   // "ROW PRIORS"
        *why = "this handle has no priors (mi355rec_sharded_set_priors)";
        return MI355REC_ERR_INVALID_ARG;
    }
    // v = fl(score + fl(beta p)): multiply, round, add, round (-ffp-contract=off); beta == 0 is the call without a prior
    const bool prior = r.prior && r.prior_weight != 0.0f;
    const float beta = r.prior_weight;
    const float* pri = prior ? h->priors.data() : nullptr;
    const Catalogue* c = h->cat;
    const int64_t n = c->n;
    std::vector<float> qn(static_cast<size_t>(k));
    for (int m = 0; m < k; ++m) qn[static_cast<size_t>(m)] = query_norm(members + m * kDim);
    std::vector<int64_t> excl;
    try {
        excl.assign(r.exclude, r.exclude + r.n_exclude);
        keys.resize(static_cast<size_t>(n));
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    std::sort(excl.begin(), excl.end());
    excl.erase(std::unique(excl.begin(), excl.end()), excl.end());
    const float* f = c->feats.data();
    // score(x) = fl(fl(...fl(fl(w_0 c_0) + fl(w_1 c_1)) + ... + fl(w_{k-1} c_{k-1})) / W), W = fl(sum |w_k|): fp32, member order,
    // multiply then add (this file is built with -ffp-contract=off), one divide.  No weights: every w_k = 1 and W = k, the
    // plain mean bit for bit.
    std::vector<float> w(static_cast<size_t>(k), 1.0f);
    if (weights) w.assign(weights, weights + k);
    const float wsum = weights ? mi355weights::sum_abs(weights, k) : static_cast<float>(k);
    // "DISTANCE REQUESTS": m(x) = fl(fl(d2_0 + ... + d2_{k-1}) / k), d2_k the sequential fp32 sum of fl(t * t), t = fl(q_kj - x_j);
    // keys carry -m, a row whose m is not finite gets no key (it is not admissible).
    const bool dist = r.metric == mi355playlist::kDistance;
    const bool anyof = r.metric == mi355playlist::kAnyOf;
    // "MANHATTAN REQUESTS": m(x) = fl(fl(d1_0 + ... + d1_{k-1}) / k), d1_k the sequential fp32 sum of fabsf(t), t = fl(q_kj - x_j);
    // keys carry -m, a row whose m is not finite gets no key (it is not admissible).
    const bool l1 = r.metric == mi355playlist::kManhattan;
    // "JACCARD REQUESTS": v(x) = fl(fl(J_0 + ... + J_{k-1}) / k), J_k = fl(num / den), num and den the sequential fp32 sums of the
    // smaller and the larger of q_kj and x_j (chosen by the one compare x_j < q_kj); keys carry v, a row whose v is not finite or
    // one of whose den is not below +inf gets no key (it is not admissible).
    const bool jaccard = r.metric == mi355playlist::kJaccard;
    // "FEATURE SCALES": two steps, as on the device: members and rows scaled with one fp32 multiply per feature, then the chains
    // above on the scaled values.  The filter below tests the stored rows f.
    const float* const a = r.scales;
    std::vector<float> scaled_members;
    if (a) {
        try {
            scaled_members.assign(members, members + static_cast<size_t>(k) * kDim);
        } catch (const std::bad_alloc&) {
            *why = "out of host memory";
            return MI355REC_ERR_OUT_OF_MEMORY;
        }
        for (int m = 0; m < k; ++m)
            for (int j = 0; j < kDim; ++j) scaled_members[static_cast<size_t>(m * kDim + j)] = a[j] * members[m * kDim + j];
        members = scaled_members.data();
        for (int m = 0; m < k; ++m) qn[static_cast<size_t>(m)] = query_norm(members + m * kDim);
    }
#pragma omp parallel for schedule(static) num_threads(c->threads)
    for (int64_t i = 0; i < n; ++i) {
        float xs[kDim];
        const float* x = f + i * kDim;   // the row the chains read: the stored one, or its scaled copy
        if (a) {
            for (int j = 0; j < kDim; ++j) xs[j] = a[j] * x[j];
            x = xs;
        }
        if (dist) {
            float sum = 0.0f;
            for (int m = 0; m < k; ++m) {
                float acc = 0.0f;
                for (int j = 0; j < kDim; ++j) {
                    const float t = members[m * kDim + j] - x[j];
                    const float sq = t * t;
                    acc = acc + sq;
                }
                sum = m == 0 ? acc : sum + acc;
            }
            const float mean = sum / static_cast<float>(k);
            keys[static_cast<size_t>(i)] = std::isfinite(mean) ? pack(-mean, static_cast<uint32_t>(i)) : 0;
            continue;
        }
        if (l1) {
            float sum = 0.0f;
            for (int m = 0; m < k; ++m) {
                float acc = 0.0f;
                for (int j = 0; j < kDim; ++j) {
                    const float t = members[m * kDim + j] - x[j];
                    acc = acc + std::fabs(t);
                }
                sum = m == 0 ? acc : sum + acc;
            }
            const float mean = sum / static_cast<float>(k);
            keys[static_cast<size_t>(i)] = std::isfinite(mean) ? pack(-mean, static_cast<uint32_t>(i)) : 0;
            continue;
        }
        if (jaccard) {
            float sum = 0.0f;
            bool bounded = true;
            for (int m = 0; m < k; ++m) {
                float num = 0.0f, den = 0.0f;
                for (int j = 0; j < kDim; ++j) {
                    const float q = members[m * kDim + j];
                    const bool lt = x[j] < q;   // (one compare, two selects: a NaN goes where the contract says)
                    num = num + (lt ? x[j] : q);
                    den = den + (lt ? q : x[j]);
                }
                bounded = bounded && den < HUGE_VALF;   // (false for NaN)
                const float jk = num / den;
                sum = m == 0 ? jk : sum + jk;
            }
            const float v = sum / static_cast<float>(k);
            keys[static_cast<size_t>(i)] = bounded && std::isfinite(v) ? pack(v, static_cast<uint32_t>(i)) : 0;
            continue;
        }
        if (anyof) {   // "ANY-OF REQUESTS": v = the best of the members' scores, in member order (the compare chain of anyof_best)
            int a;
            keys[static_cast<size_t>(i)] = pack(anyof_best(members, qn.data(), k, x, &a), static_cast<uint32_t>(i));
            continue;
        }
        float sum = w[0] * score(members, qn[0], x);
        for (int m = 1; m < k; ++m) {
            const float term = w[static_cast<size_t>(m)] * score(members + m * kDim, qn[static_cast<size_t>(m)], x);
            sum = sum + term;
        }
        float v = sum / wsum;
        if (prior) {
            const float b = beta * pri[i];
            v = v + b;
        }
        keys[static_cast<size_t>(i)] = pack(v, static_cast<uint32_t>(i));
    }
    for (int64_t e : excl)
        if (e >= 0 && e < n) keys[static_cast<size_t>(e)] = 0;   // (a real key is never 0: its low half is ~row)
    int64_t avail = n - static_cast<int64_t>(std::count_if(excl.begin(), excl.end(), [n](int64_t e) { return e >= 0 && e < n; }));
    if (dist || l1 || jaccard) avail =static_cast<int64_t>(std::count_if(keys.begin(), keys.end(), [](uint64_t key) { return key != 0; }));
    if (filter && filter->active) {   // the rows failing the filter go like excluded ones
        avail = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t& key = keys[static_cast<size_t>(i)];
            if (key != 0 && !mi355filter::pass(filter, f + i * kDim)) key = 0;
            avail += key != 0;
        }
    }
    if (r.n_labels > 0) {   // ... and so do the rows whose label is not in the set (-1: never)
        uint32_t mask[MI355REC_MAX_LABELS / 32];
        mi355playlist::label_bits(r, mask);
        const LabelFilter in_set{h->labels.data(), mask};
        avail = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t& key = keys[static_cast<size_t>(i)];
            if (key != 0 && !in_set.keeps(i)) key = 0;
            avail += key != 0;
        }
    }
    if (r.rowset) {   // "ROW SETS": ... and the rows the set does not admit (rowset.h: the host bitmap, global rows)
        avail = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t& key = keys[static_cast<size_t>(i)];
            if (key != 0 && !mi355rowset::admits(r.rowset, r.rowset_only, i)) key = 0;
            avail += key != 0;
        }
    }
    if (r.listed) {   // "CANDIDATE LISTS": ... and the rows that are not listed (candidates.h: the sorted list, searched per row)
        std::vector<uint32_t> listed;
        try {
            listed.resize(static_cast<size_t>(r.n_candidates > 0 ? r.n_candidates : 1));
        } catch (const std::bad_alloc&) {
            *why = "out of host memory";
            return MI355REC_ERR_OUT_OF_MEMORY;
        }
        const int64_t n_listed = mi355cand::reduce(r.candidates, r.n_candidates, 0, n, listed.data()).count;
        avail = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t& key = keys[static_cast<size_t>(i)];
            if (key != 0 && !mi355cand::contains(listed.data(), n_listed, i)) key = 0;
            avail += key != 0;
        }
    }
    *admissible = avail;
    return MI355REC_OK;
}

int node_query_mean(Node* h, const mi355playlist::Request& r, const mi355playlist::Outputs& out, const char** why) {
    const int topn_asked = r.topn;
    std::vector<uint64_t> keys;
    int64_t avail = 0;
    const int rc = mean_keys(h, r, keys, &avail, why);
    if (rc) return rc;
    if (r.bounded) {   // "BOUNDED REQUESTS": only the keys above the floor are left; their number is the total
        avail = 0;
        for (uint64_t& key : keys) {
            if (key <= r.floor_thr) key = 0;
            avail += key != 0;
        }
        *out.total = avail;
    }
    const int count = static_cast<int>(topn_asked < avail ? topn_asked : avail);
    std::partial_sort(keys.begin(), keys.begin() + count, keys.end(), std::greater<uint64_t>());
    for (int i = 0; i < count; ++i) {
        out.idx[i] = static_cast<int64_t>(~static_cast<uint32_t>(keys[static_cast<size_t>(i)]));
        if (out.score) out.score[i] = unordered(static_cast<uint32_t>(keys[static_cast<size_t>(i)] >> 32)) + 0.0f;
        if (out.member) {   // "ANY-OF REQUESTS": the matched member of a result row: its k chains once more
            float qn[MI355REC_MAX_PLAYLIST];
            for (int m = 0; m < r.k; ++m) qn[m] = query_norm(r.members + m * kDim);
            int a = 0;
            (void)anyof_best(r.members, qn, r.k, h->cat->feats.data() + out.idx[i] * kDim, &a);
            out.member[i] = a;
        }
    }
    if (topn_asked > 0) mi355playlist::pad(out, count, topn_asked, count);
    else if (out.count) *out.count = 0;   // ("BOUNDED REQUESTS", count only: out.idx may be null)
    if (r.report_distance && topn_asked > 0) mi355playlist::scores_to_distances(out, topn_asked, r.metric);
    return MI355REC_OK;
}

// CANDIDATE SCORES (include/mi355rec_diag.h): the same keys, read at every listed id in list order (the ids are checked: rows of the catalogue).
int node_score_rows(Node* h, const mi355playlist::Request& r, const mi355playlist::ScoreOutputs& out, const char** why) {
    std::vector<uint64_t> keys;
    int64_t avail = 0;
    const int rc = mean_keys(h, r, keys, &avail, why);
    if (rc) return rc;
    for (int64_t i = 0; i < r.n_candidates; ++i) {
        const uint64_t key = keys[static_cast<size_t>(r.candidates[i])];
        if (key) mi355playlist::score_some(r, out, i, unordered(static_cast<uint32_t>(key >> 32)) + 0.0f);
        else mi355playlist::score_none(out, i);
    }
    return MI355REC_OK;
}

// DIVERSIFIED TOP-N (include/mi355rec_diag.h): the pool is node_query_mean's top-`pool`; then the greedy picks, a plain loop
// over P' <= 1024 rows.  mmr = fl(fl(lambda rel) - fl(mu pen)): multiply, round, subtract, round (-ffp-contract=off).
int node_query_mean_diverse(Node* h, const mi355playlist::Request& r, const mi355playlist::Outputs& out, const char** why) {
    const bool capped = r.capped;   // GROUP CAPS
    const float lambda = r.lambda;
    const int pool = r.pool, topn = r.topn, max_per_group = r.max_per_group;
    if (out.pool_rows) *out.pool_rows = 0;
    if (capped && !h->has_groups) {
        *why = "this handle has no groups (mi355rec_sharded_set_groups)";
        return MI355REC_ERR_INVALID_ARG;
    }
    std::vector<int64_t> pidx;
    std::vector<float> prel, pen, qn;
    std::vector<char> picked;
    std::vector<int> seen;   // per pool row: the picked rows of its group so far
    try {
        if (capped) seen.assign(static_cast<size_t>(pool), 0);
        pidx.resize(static_cast<size_t>(pool));
        prel.resize(static_cast<size_t>(pool));
        pen.assign(static_cast<size_t>(pool), 0.0f);
        qn.resize(static_cast<size_t>(pool));
        picked.assign(static_cast<size_t>(pool), 0);
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    int p_eff = 0;
    const int rc = node_query_mean(h, r.pool_call(), {pidx.data(), prel.data(), nullptr, &p_eff, nullptr}, why);
    if (rc != MI355REC_OK) return rc;
    if (out.pool_rows) *out.pool_rows = p_eff;
    const float* f = h->cat->feats.data();
    const float mu = 1.0f - lambda;
    int picks = topn < p_eff ? topn : p_eff;   // (capped: at most so many)
    auto group_of = [&](int i) { return h->groups[static_cast<size_t>(pidx[static_cast<size_t>(i)])]; };
    for (int i = 0; i < p_eff; ++i) qn[static_cast<size_t>(i)] = query_norm(f + pidx[static_cast<size_t>(i)] * kDim);
    for (int t = 0; t < topn; ++t) {
        if (t >= picks) {
            out.idx[t] = -1;
            if (out.score) out.score[t] = 0.0f;
            if (out.mmr) out.mmr[t] = 0.0f;
            continue;
        }
        int best = -1;
        float best_mmr = 0.0f;
        for (int i = 0; i < p_eff; ++i) {
            if (picked[static_cast<size_t>(i)]) continue;
            if (capped && group_of(i) >= 0 && seen[static_cast<size_t>(i)] >= max_per_group) continue;   // not eligible
            const float a = lambda * prel[static_cast<size_t>(i)];
            const float b = mu * pen[static_cast<size_t>(i)];
            const float mmr = a - b;
            if (best < 0 || mmr > best_mmr) {   // IEEE >: a tie stays with the earlier pool position
                best = i;
                best_mmr = mmr;
            }
        }
        if (best < 0) {   // (capped only) nothing is eligible: the loop ends, the rest is padding
            picks = t;
            --t;
            continue;
        }
        picked[static_cast<size_t>(best)] = 1;
        if (capped && group_of(best) >= 0)
            for (int i = 0; i < p_eff; ++i) seen[static_cast<size_t>(i)] += group_of(i) == group_of(best);
        out.idx[t] = pidx[static_cast<size_t>(best)];
        if (out.score) out.score[t] = prel[static_cast<size_t>(best)];
        if (out.mmr) out.mmr[t] = best_mmr;
        const float* q = f + pidx[static_cast<size_t>(best)] * kDim;
        for (int i = 0; i < p_eff; ++i) {
            if (picked[static_cast<size_t>(i)]) continue;
            const float c = score(q, qn[static_cast<size_t>(best)], f + pidx[static_cast<size_t>(i)] * kDim);   // row i scanned, row p the query
            if (c > pen[static_cast<size_t>(i)]) pen[static_cast<size_t>(i)] = c;
        }
    }
    if (out.count) *out.count = picks;
    return MI355REC_OK;
}

int node_set_window(Node* h, int window, const char** why) {
    if (window < 1 || window > kMaxWindow) {
        *why = "window out of range";
        return MI355REC_ERR_INVALID_ARG;
    }
    if (window == h->window) return MI355REC_OK;
    node_flush(h);
    h->next_ticket = (h->next_ticket + window - 1) / window * window;
    h->window = window;
    h->s_topn = 0;   // buffers are re-made by the next enqueue
    for (auto& w : h->win) w = Node::Win();
    return MI355REC_OK;
}

int node_enqueue(Node* h, const float* q12, int64_t exclude, int topn_asked, int64_t* ticket, const char** why) {
    if (topn_asked <= 0 || topn_asked > MI355REC_MAX_TOPN_FAST) {
        *why = "topn must be in [1, 1024] for streamed queries";
        return MI355REC_ERR_INVALID_ARG;
    }
    const int64_t t0 = now_ns();
    const int W = h->window;
    if (h->s_topn != topn_asked) {   // a change of geometry closes the stream; tickets keep growing, window-aligned
        node_flush(h);
        h->s_topn = 0;
        try {
            h->idx.assign(static_cast<size_t>(kDepth) * W * topn_asked, -1);
            h->score.assign(static_cast<size_t>(kDepth) * W * topn_asked, 0.0f);
            h->counts.assign(static_cast<size_t>(kDepth) * W, 0);
        } catch (const std::bad_alloc&) {
            *why = "out of host memory";
            return MI355REC_ERR_OUT_OF_MEMORY;
        }
        h->s_topn = topn_asked;
        for (auto& w : h->win) w = Node::Win();
    }
    const int64_t t = h->next_ticket;
    const int64_t abs = t / W;
    const int w = static_cast<int>(abs % kDepth);
    const int slot = static_cast<int>(t % W);
    if (slot == 0) {
        h->win[w].abs = abs;
        h->win[w].count = 0;
        ++h->st_windows;
    }
    const size_t at = (static_cast<size_t>(w) * W + slot) * topn_asked;
    int c = 0;
    try {
        c = topn(h->cat, q12, exclude, topn_asked, &h->idx[at], &h->score[at]);
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    for (int i = c; i < topn_asked; ++i) {
        h->idx[at + i] = -1;
        h->score[at + i] = 0.0f;
    }
    h->counts[static_cast<size_t>(w) * W + slot] = c;
    ++h->win[w].count;
    ++h->next_ticket;
    ++h->st_queries;
    if (ticket) *ticket = t;
    h->st_ns += now_ns() - t0;
    return MI355REC_OK;
}

int node_flush(Node* h) {   // nothing is ever pending; the next query opens a new window, as on the GPU path
    const int W = h->window;
    h->next_ticket = (h->next_ticket + W - 1) / W * W;
    return MI355REC_OK;
}

int node_wait(Node* h, int64_t ticket, int64_t* out_idx, float* out_score, int* out_count, const char** why) {
    if (!h->s_topn || ticket < 0 || ticket >= h->next_ticket) {
        *why = "ticket was never handed out";
        return MI355REC_ERR_INVALID_ARG;
    }
    const int W = h->window;
    const int64_t abs = ticket / W;
    const int w = static_cast<int>(abs % kDepth);
    const int slot = static_cast<int>(ticket % W);
    if (h->win[w].abs != abs || slot >= h->win[w].count) {
        *why = "the results of this ticket are no longer kept (ring of 4 windows)";
        return MI355REC_ERR_INVALID_ARG;
    }
    const size_t at = (static_cast<size_t>(w) * W + slot) * h->s_topn;
    std::memcpy(out_idx, &h->idx[at], sizeof(int64_t) * h->s_topn);
    if (out_score) std::memcpy(out_score, &h->score[at], sizeof(float) * h->s_topn);
    if (out_count) *out_count = h->counts[static_cast<size_t>(w) * W + slot];
    return MI355REC_OK;
}

void node_stream_stats(const Node* h, int64_t* queries, int64_t* windows, int64_t* host_ns) {
    if (queries) *queries = h->st_queries;
    if (windows) *windows = h->st_windows;
    if (host_ns) *host_ns = h->st_ns;
}

}  // namespace mi355cpu
