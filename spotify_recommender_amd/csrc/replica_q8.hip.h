// replica_q8.hip.h — the 8-BIT replica of the catalogue and the single-query scan over it.
//
// replica.hip.h halves the bytes a query streams (24 B per row instead of the reference's 48,
// Recommender.cu:184-254) with a copy that is only good enough to rule rows OUT.  The same idea one step
// further: 12 B per row.  Each row is L2-normalised in fp32 and every component quantised to a SIGNED byte,
//     k_j = round(127 r^_j)   in [-127, 127],          |k_j - 127 r^_j| <= 1/2,
// and the query (normalised q^ = q / |q|) to 16 bits, held as two balanced int8 digits per component,
//     Q_j = round(S q^_j) = 256 h_j + l_j,   S = 32000,   h_j in [-125, 125],   l_j in [-128, 127],
// so that the dot product the reference takes with cublasSgemv (Recommender.cu:217-223) is, for ruling rows out,
// SIX v_dot4_i32_i8 per row — three over the high digits, three over the low ones — and one shift-add:
//     D = sum_j k_j Q_j = 256 sum_j k_j h_j + sum_j k_j l_j          (int32, exact: |D| < 4.2e6)
//     approx = D / (127 S),        approx - r^ . q^ = sum_j (k_j/127 - r^_j) Q_j/S + sum_j r^_j (Q_j/S - q^_j)
//     |approx - r^ . q^| <= l1(Q) / (254 S) + l1(r^) / (2 S) <= l1(Q) / (254 S) + sqrt(12) / (2 S).
// (Until round 5 the query stayed fp32 and a row cost 12 v_cvt_f32_ubyte + 12 v_fmac: 96 vector instructions per lane
// and 48 B, which kept the kernel at 0.75 of a plain read of its own buffer.)  The candidate test itself is an INTEGER
// compare: a row is out iff D < floor(cutoff * 127 S) - 1 (q8_threshold: the fp32 product is off by < 0.25).
// The bound is PER QUERY (0.0137 at worst, ~0.012 for a typical query) and derived, not tuned: the row's
// quantisation error of component j is at most 1/254 and enters multiplied by |Q_j| / S, the query's is at most
// 1 / (2 S) and enters multiplied by |r^_j| (5.5e-5 in all); the normalisations in fp32 (v_rsq_f32: the byte may sit
// 4e-5 of a step off its real-number position), the one rounding of D / (127 S) where a float is wanted and the
// reference chain's own rounding are covered by kQ8Slack = 3e-5 (together < 8e-6).  tests/test_q8_margin.py checks
// it on hostile data with a numpy model of exactly this arithmetic.  Everything else is replica.hip.h's scheme:
//   * the contract per query is recommendByIndex's (Recommender.cu:275-318): every key that leaves the
//     kernel is cosine_score() on the fp32 row (calculateSimilaritiesCPU, :256-273), bit for bit;
//   * valid row: |row|^2 in [kBqMinNorm2, kBqMaxNorm2]; an exactly-zero row stores k = 0 everywhere
//     (approx = 0 = its exact score); every other row (tiny, huge, inf, NaN) stores 0x80 = -128 — a byte no
//     valid row contains — and is sent to the exact chain every time;
//   * an invalid query (|q| outside [kBqMinNorm, kBqMaxNorm]) switches the pre-filter off for the launch;
//   * the launch-wide cutoff comes from a spread sample of 256-row wave tiles (5 % of the catalogue): per tile the
//     EXACT score of the row with the largest approx (q8_region_pick / q8_region_store); v = the topk-th largest of
//     those <= 2048 exact scores, cutoff = v - margin (ONE margin: v is the exact score of a real row; shards too
//     small to afford the extra fetch keep approximate sample values and two margins); workgroup-local thresholds
//     tighten it whenever a local list fills;
//   * ... or, where the handle was told to (mi355rec_set_sample), from the BUCKETED sample: a fifth of the rows grouped by
//     direction once, beside the replica, of which a query reads 32 regions whose buckets lie nearest to it — 0.8 MB instead of 6.3 MB,
//     one exact score per 64 rows ("the bucketed sample" below).  Half the candidates of the strided sample at 10 M rows.
// With a margin twelve times the fp16 replica's, ~0.1 % of the rows (~9 000 of 10 M at top-100) go to the exact
// chain instead of 0.05 % — 0.6 MB of random 48 B fetches beside 120 MB of stream.
//
// One lane = FOUR rows = 48 B (3 x dwordx4: the same load pattern once more; row r of the lane is dwords
// 3r .. 3r + 2), tiles of 4 * kBlock rows dealt round-robin over the scanning workgroups.
//
// -DMI355_Q8_QUERY_BITS=8 (A/B builds only) quantises the query to ONE int8 digit, P_j = round(127 q^_j): three
// v_dot4 per row, and a margin of l1(P) / (254 * 127) + sqrt(12) / 254 — twice the rows to the exact chain.
#pragma once

#include "replica.hip.h"

#ifndef MI355_Q8_QUERY_BITS
#define MI355_Q8_QUERY_BITS 16
#endif

namespace mi355 {

constexpr int kQ8QueryBits = MI355_Q8_QUERY_BITS;
static_assert(kQ8QueryBits == 16 || kQ8QueryBits == 8, "the query is one or two int8 digits per component");
constexpr float kQ8Step = 1.0f / 254.0f;     // half a quantisation step of a normalised row component
constexpr float kQ8QueryScale = kQ8QueryBits == 16 ? 32000.0f : 127.0f;   // S: Q_j = round(S q^_j)
constexpr float kQ8DotScale = 127.0f * kQ8QueryScale;                      // approx = D / (127 S)
constexpr float kQ8QueryResidual = 3.4642f * 0.5f / kQ8QueryScale;         // l1(r^) / (2 S), l1(r^) <= sqrt(12)
constexpr float kQ8Slack = 3e-5f;            // fp32 normalisations of row and query, the byte's rsq-induced offset, the rounding of
                                             // D / (127 S) and the reference chain's own rounding (together < 8e-6), with room to spare
constexpr uint32_t kQ8Special = 0x80u;       // first byte of a row the bound is not claimed for (-128: no valid row holds it)

// ---- building the replica ---------------------------------------------------------------------------
// One thread per row; rows [n, n_padded) (n_padded a multiple of 4) are padding and hold the special marker.
// q8 and norms may each be null (uniform tests): the replica is stored only where q8 is given; where norms is given,
// norms[row] = sqrtf of the SEQUENTIAL fp32 sum of squares (multiply, round, add, round: what query_norm computes; 0.0f for
// the padding) — the per-row norms of the distance requests (playlist.hip.h, "DISTANCE"), 4 B per row in local row order.
// The same kernel builds what the BUCKETED SAMPLE keeps beside the replica ("the bucketed sample" below; one kernel, not
// three: the library's kernel count is capped):
//   * pick != null: thread e works on local row pick[e] instead of row e (outside [0, n): padding) and stores at index e —
//     the base rows' entries in sample order;
//   * centroids != null: bucket[e] = the centroid with the largest dot product row . c / |c| (the row's own norm scales
//     every candidate alike): a sequential fma chain in feature order and centroid order, so deterministic, and a tie
//     keeps the LOWER centroid (strict >).  A centroid whose norm is zero or not finite counts as score 0.
//   * upd_dst != null — the UPDATE job (mi355rec_update_rows, engine_update.hip.h): thread e reads source row upd_src[e] (row e
//     where upd_src is null: the staged rows of the call) of `feats`, which holds n rows, and stores at row upd_dst[e] instead of
//     slot e: the 8-bit entry, the fp16 entry (half), the norm and the fp32 row itself (rows_out), each where its pointer is
//     given.  n_padded is the number of rows of the call; padding is never written.  The label-grouped copy is the same job
//     with only rows_out and upd_dst = the rows' sorted positions.  half and rows_out are null in every other job.

// The 8-bit entry of a row (three dwords; tot = replica_norm2 of it): left as it is — the special marker — unless the row is
// valid or exactly zero.
__device__ __forceinline__ void q8_pack_row(const float4& a, const float4& b, const float4& c, float tot, uint32_t& d0, uint32_t& d1,
                                            uint32_t& d2) {
    const bool valid = tot >= kBqMinNorm2 && tot <= kBqMaxNorm2;
    if (valid || tot == 0.0f) {
        const float inv = valid ? __builtin_amdgcn_rsqf(tot) * 127.0f : 0.0f;
        auto q = [&](float x) {   // round to nearest; |x * inv| <= 127 (1 + 1e-6); two's complement byte
            int k = static_cast<int>(__builtin_rintf(x * inv));
            k = k > 127 ? 127 : (k < -127 ? -127 : k);
            return static_cast<uint32_t>(k) & 0xffu;
        };
        d0 = q(a.x) | (q(a.y) << 8) | (q(a.z) << 16) | (q(a.w) << 24);
        d1 = q(b.x) | (q(b.y) << 8) | (q(b.z) << 16) | (q(b.w) << 24);
        d2 = q(c.x) | (q(c.y) << 8) | (q(c.z) << 16) | (q(c.w) << 24);
    }
}

__global__ __launch_bounds__(256) void q8_build_kernel(const float* __restrict__ feats, int64_t n, int64_t n_padded,
                                                       uint32_t* __restrict__ q8, float* __restrict__ norms,
                                                       const int32_t* __restrict__ pick, const float* __restrict__ centroids,
                                                       int n_centroids, int32_t* __restrict__ bucket,
                                                       const int64_t* __restrict__ upd_src, const int64_t* __restrict__ upd_dst,
                                                       uint2* __restrict__ half, float* __restrict__ rows_out) {
    __shared__ float s_inv[1024];
    if (centroids) {   // uniform
        n_centroids = n_centroids < 1024 ? n_centroids : 1024;
        for (int c = threadIdx.x; c < n_centroids; c += blockDim.x) {
            float tot = 0.0f;
            for (int j = 0; j < kDim; ++j) tot = __builtin_fmaf(centroids[c * kDim + j], centroids[c * kDim + j], tot);
            const float inv = 1.0f / sqrtf(tot);
            s_inv[c] = (tot > 0.0f && inv == inv && inv < 3.0e38f) ? inv : 0.0f;
        }
        __syncthreads();
    }
    const int64_t slot = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (slot >= n_padded) return;
    int64_t row = slot, out = slot;
    if (pick) {   // uniform
        row = pick[slot];
        row = row >= 0 ? row : n;   // (padding)
    }
    if (upd_dst) {   // uniform: the update job
        row = upd_src ? upd_src[slot] : slot;
        out = upd_dst[slot];
        if (row < 0 || row >= n) return;   // (the host has checked the list: an update never writes padding)
    }
    uint32_t d0 = 0x80808080u, d1 = 0x80808080u, d2 = 0x80808080u;   // special
    uint32_t hp[6] = {kHalfNaN2, kHalfNaN2, kHalfNaN2, kHalfNaN2, kHalfNaN2, kHalfNaN2};
    float seq = 0.0f;
    if (row < n) {
        const float4* p = reinterpret_cast<const float4*>(feats) + row * 3;
        const float4 a = p[0], b = p[1], c = p[2];
        if (rows_out) {   // uniform
            float4* dst = reinterpret_cast<float4*>(rows_out) + out * 3;
            dst[0] = a;
            dst[1] = b;
            dst[2] = c;
        }
        if (centroids) {   // uniform
            const float f[kDim] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            float best = -__builtin_inff();
            int best_c = 0;
            for (int k = 0; k < n_centroids; ++k) {   // (uniform addresses: scalar loads)
                float dot = 0.0f;
#pragma unroll
                for (int j = 0; j < kDim; ++j) dot = __builtin_fmaf(f[j], centroids[k * kDim + j], dot);
                const float v = dot * s_inv[k];
                if (v > best) {
                    best = v;
                    best_c = k;
                }
            }
            bucket[slot] = best_c;
        }
        if (norms) {   // uniform
            const float f[kDim] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int j = 0; j < kDim; ++j) seq = seq + f[j] * f[j];
        }
        // the normalisation of the fp16 replica and of the batched passes (replica_norm2, replica.hip.h)
        const float tot = replica_norm2(a, b, c);
        q8_pack_row(a, b, c, tot, d0, d1, d2);
        if (half) half_pack_row(a, b, c, tot, hp);   // uniform
    } else if (centroids) {   // uniform
        bucket[slot] = 0;     // (padding: any bucket in range)
    }
    if (q8) {   // uniform
        uint32_t* dst = q8 + out * 3;
        dst[0] = d0;
        dst[1] = d1;
        dst[2] = d2;
    }
    if (half) {   // uniform
        uint2* dst = half + out * 3;
        dst[0] = make_uint2(hp[0], hp[1]);
        dst[1] = make_uint2(hp[2], hp[3]);
        dst[2] = make_uint2(hp[4], hp[5]);
    }
    if (norms) norms[out] = sqrtf(seq);   // uniform
}

// ---- the query ------------------------------------------------------------------------------------------
struct Q8Query {
    int hi[3];       // the high int8 digits h_j, four per dword in the row's byte order (wave-uniform: scalar registers)
    int lo[3];       // the low digits l_j (16-bit query only)
    float inv;       // 1 / (127 S):   approx = D * inv
    float margin;    // l1(Q) / (254 S) + l1(r^) / (2 S) + slack
    bool ok;         // the bound may be claimed for this query
};

__device__ __forceinline__ Q8Query q8_query(const float (&q)[kDim], float qn) {
    Q8Query r;
    r.ok = qn >= kBqMinNorm && qn <= kBqMaxNorm;   // false for NaN
    const float inv = r.ok ? 1.0f / qn : 0.0f;
    r.hi[0] = r.hi[1] = r.hi[2] = 0;
    r.lo[0] = r.lo[1] = r.lo[2] = 0;
    int l1 = 0;
    constexpr int kMax = static_cast<int>(kQ8QueryScale);
#pragma unroll
    for (int j = 0; j < kDim; ++j) {
        int Q = static_cast<int>(__builtin_rintf(q[j] * inv * kQ8QueryScale));   // |q^_j| <= 1 + 1e-6
        Q = Q > kMax ? kMax : (Q < -kMax ? -kMax : Q);
        l1 += Q < 0 ? -Q : Q;
        if constexpr (kQ8QueryBits == 16) {
            const int h = (Q + 128) >> 8;      // balanced digits: Q = 256 h + l, l in [-128, 127], |h| <= 125
            const int l = Q - 256 * h;
            r.hi[j >> 2] |= (h & 0xff) << (8 * (j & 3));
            r.lo[j >> 2] |= (l & 0xff) << (8 * (j & 3));
        } else {
            r.hi[j >> 2] |= (Q & 0xff) << (8 * (j & 3));
        }
    }
    r.inv = 1.0f / kQ8DotScale;
    r.margin = static_cast<float>(l1) * (kQ8Step / kQ8QueryScale) * (1.0f + 1e-5f) + kQ8QueryResidual + kQ8Slack;
    return r;
}

// D of one row (3 dwords); `special` = the row is sent to the exact chain whatever D says
__device__ __forceinline__ int q8_dot(const Q8Query& q, uint32_t d0, uint32_t d1, uint32_t d2, bool& special) {
    special = (d0 & 0xffu) == kQ8Special;
    int hi = __builtin_amdgcn_sdot4(static_cast<int>(d0), q.hi[0], 0, false);
    hi = __builtin_amdgcn_sdot4(static_cast<int>(d1), q.hi[1], hi, false);
    hi = __builtin_amdgcn_sdot4(static_cast<int>(d2), q.hi[2], hi, false);
    if constexpr (kQ8QueryBits == 16) {
        int lo = __builtin_amdgcn_sdot4(static_cast<int>(d0), q.lo[0], 0, false);
        lo = __builtin_amdgcn_sdot4(static_cast<int>(d1), q.lo[1], lo, false);
        lo = __builtin_amdgcn_sdot4(static_cast<int>(d2), q.lo[2], lo, false);
        return (hi << 8) + lo;   // (v_lshl_add_u32)
    } else {
        return hi;
    }
}

__device__ __forceinline__ void q8_dot4(const Q8Query& q, const HalfTile& t, int (&a)[4], bool (&special)[4]) {
    a[0] = q8_dot(q, t.t0.x, t.t0.y, t.t0.z, special[0]);
    a[1] = q8_dot(q, t.t0.w, t.t1.x, t.t1.y, special[1]);
    a[2] = q8_dot(q, t.t1.z, t.t1.w, t.t2.x, special[2]);
    a[3] = q8_dot(q, t.t2.y, t.t2.z, t.t2.w, special[3]);
}

// approx as a float (samples, diagnostics): |D| < 2^24 converts exactly, one rounding in the product
__device__ __forceinline__ float q8_approx(const Q8Query& q, int d) { return static_cast<float>(d) * q.inv; }

// The integer image of a cutoff: a row whose D is below it has approx < cutoff.  The fp32 product cutoff * 127 S is off
// by < 0.25 (|cutoff| <= 2: 2^-24 relative of at most 8.2e6), floor(...) - 1 stays below the real-number product.
// -inf / NaN (no bound) => INT_MIN: every row is a candidate.
__device__ __forceinline__ int q8_threshold(float cutoff) {
    if (!(cutoff > -2.0f)) return static_cast<int>(0x80000000u);
    const float c = cutoff < 2.0f ? cutoff : 2.0f;
    return static_cast<int>(__builtin_floorf(c * kQ8DotScale)) - 1;
}

// ---- the sample that seeds the launch-wide cutoff ---------------------------------------------------------
// A REGION is 2048 rows from row g * stride_rows on (stride_rows a multiple of 4 and >= 2048): one ordered-u32
// approx maximum per 256-row wave tile (0 = nothing usable) goes to seed_vals[g * 8 + wave].
struct Q8Region {
    HalfTile t;
    int64_t quad;
    bool have;
};

__device__ __forceinline__ Q8Region q8_region_load(const uint4* __restrict__ q8, int64_t n_quads, int64_t stride_rows, int64_t g) {
    Q8Region s;
    s.quad = ((g * stride_rows) >> 2) + threadIdx.x;
    s.have = s.quad < n_quads;
    s.quad = s.have ? s.quad : n_quads - 1;
    const uint4* p = q8 + s.quad * 3;
    s.t.t0 = p[0];
    s.t.t1 = p[1];
    s.t.t2 = p[2];
    return s;
}

// The sample value of one wave's 256 rows is the EXACT score of the row whose approximate score is the largest
// (one 48 B fetch per wave, all lanes the same address): an exact score v of a real row needs only ONE margin in
// the cutoff (approx < v - margin => exact < v), where the approximate maximum needed two.  At top-100 over
// 10 M rows that is the difference between ~28 000 and ~10 000 rows sent to the exact chain per query.
// (exact = false keeps the approximate maximum and skips the fetch: small shards, where the riders' extra round
// trip is on the critical path of the launch and a few hundred more candidates are not.)
struct Q8Pick {
    int64_t row;     // wave-uniform: local row of the wave's best usable row
    uint32_t top;    // wave-uniform: its approximate score, ordered (0: no usable row)
    bool any;        // wave-uniform
};

__device__ __forceinline__ Q8Pick q8_region_pick(const Q8Region& s, const Q8Query& q, int64_t n, int64_t row_base,
                                                 int64_t exclude_global) {
    int a[4];
    bool special[4];
    q8_dot4(q, s.t, a, special);
    const int64_t r0 = s.quad * 4;
    uint32_t v = 0u;
    int best = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool use = s.have && q.ok && !special[u] && r0 + u < n && row_base + r0 + u != exclude_global;
        const uint32_t w = use ? score_to_ordered(q8_approx(q, a[u])) : 0u;
        best = w > v ? u : best;
        v = w > v ? w : v;
    }
    const uint32_t top = wave_max_u32(v);
    const uint64_t holders = __ballot(v == top);   // never empty
    const int lane = static_cast<int>(__builtin_ctzll(holders));
    Q8Pick p;
    p.top = top;
    p.any = top != 0u;
    const int64_t mine = r0 + best;
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(mine)), lane));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(mine >> 32)), lane));
    p.row = p.any ? static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo) : 0;
    return p;
}

__device__ __forceinline__ void q8_region_store(const Q8Pick& p, const Row& row, const float (&q)[kDim], float qn,
                                                unsigned long long* __restrict__ seed_vals, uint32_t epoch, int64_t g, bool exact) {
    uint32_t v = p.top;
    if (exact) {   // (uniform)
        const float exact = cosine_score(q, qn, row);
        v = p.any ? score_to_ordered(exact) : 0u;
    }
    // written THROUGH to device scope, under the query's epoch: a rider of the same launch may read it
    // (scan_q8_kernel, last rider out; replica.hip.h, "hand-offs that fail safe")
    if ((threadIdx.x & 63) == 0)
        __hip_atomic_store(&seed_vals[g * kHalfSeedWaves + (threadIdx.x >> 6)], tag_value(epoch, v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void q8_load_query(const float* __restrict__ query_ptr, const float (&by_value)[kDim], float (&q)[kDim]) {
    if (query_ptr) {
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = query_ptr[j];
    } else {
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = by_value[j];
    }
}

// ---- the bucketed sample ------------------------------------------------------------------------------------------
// The strided sample reads 256 regions x 2048 rows (5 % of a 10 M-row catalogue, 6.3 MB) for EVERY query and keeps the
// best row of each 256-row wave tile, wherever the query points.  Which rows are worth looking at depends on the query's
// direction, and the catalogue does not change between queries — so the grouping is done once, beside the replica
// (engine_state.hip.h, build_bucket_sample): a BASE of up to 1024 strided regions (a fifth of the rows) is assigned, row by
// row, to the nearest of as many CENTROIDS (strided catalogue rows, largest normalised dot product, ties to the lower
// centroid), ordered by (bucket, row) on the host (bucket_sample.h) and kept as a contiguous copy of the rows' 12 B
// entries + their local row numbers + the bucket range of every 2048-row region of that order.  A query then
//   1. scores the centroids (exact chain, <= 2 per thread), gives every region the best centroid score of its bucket
//      range (its first kBucketSpanMax - 1 buckets and its last: a longer range only happens where buckets are nearly empty) and
//      takes the regions whose score reaches the picks-th best one, the first `picks` of them in region order;
//   2. reads those `picks` <= 32 regions (0.79 MB instead of 6.3), riders taking every n_wgs-th of them.  The selection
//      returns the lower edge of a histogram bin, so a few more than `picks` regions can reach it: kept are the first
//      `picks` in region order, all of them within one bin (2.4e-4) of the picks-th best score — not the best by rank;
//   3. takes one value per 64 rows of a region — the 16 lanes of a DPP row x 4 rows per lane: the lane that holds the
//      row's best approximate score looks its row up (BucketSample::rows), fetches it from the CURRENT fp32 matrix and
//      stores cosine_score() of it — up to 32 x 32 = 1024 values at out[rank * 32 + tid / 16].
// Every rider redoes 1.: the same arithmetic on the same table gives the same ranking, so the riders' shares are
// disjoint without a hand-off between them.  What decides RESULTS is only that every value is the exact score of a
// real, distinct, eligible row of this shard: entries are distinct rows (a permutation of the base), padding holds the
// special marker and row -1, the excluded row and rows outside [0, n) yield nothing, an invalid query yields nothing.
// Poorly chosen regions (a stale copy after rows changed in place, a degenerate centroid) only loosen the bound.
constexpr int kBucketMaxRegions = 1024;   // regions of the base, and centroids
constexpr int kBucketPicks = 32;          // regions a query reads
constexpr int kBucketGroups = kHalfSeedBlock / 16;   // values per region: one per DPP row of 16 lanes
constexpr int kBucketSpanMax = 8;         // buckets of a region's range that are looked at: the first 7 and the last (a loop over
                                          // the whole range was 64 dependent LDS reads in some thread of every rider: ~3 us)
constexpr int kBucketAhead = 4;           // regions of a rider in flight
constexpr int kBucketScratch = kBucketMaxRegions + kSelScratch + kBucketPicks + 8 + 1;   // ints of LDS scratch
static_assert(kBucketPicks * kBucketGroups <= kHalfSeedPerThread * kHalfSeedBlock, "the values fit the sample buffer's selection");

// Called by all kHalfSeedBlock threads of sampling workgroup `rider` of `n_wgs`.  `s`: kBucketScratch ints of LDS nobody
// else is using, `sel`: the selection's histogram.  drop (test hook): nothing is stored.
__device__ __forceinline__ Q8Query q8_bucket_sample(const float* __restrict__ feats, const BucketSample& bs, int64_t n, int64_t row_base,
                                                    const float* __restrict__ query_ptr, const float (&by_value)[kDim],
                                                    int64_t exclude_global, unsigned long long* __restrict__ out, uint32_t epoch,
                                                    int rider, int n_wgs, bool drop, int* s, SelectSmem& sel) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    uint32_t* const s_cent = reinterpret_cast<uint32_t*>(s);   // [kBucketMaxRegions] centroid scores, ordered
    int* const s_bins = s + kBucketMaxRegions;                  // [kSelScratch] the selection's scratch
    int* const s_pick = s_bins + kSelScratch;                   // [kBucketPicks] the regions to read (-1: none)
    int* const s_wave = s_pick + kBucketPicks;                  // [8] per-wave counts of the prefix sum
    int* const s_count = s_wave + 8;                            // [1] the selection's counter
    const int n_cent = bs.n_centroids < kBucketMaxRegions ? bs.n_centroids : kBucketMaxRegions;
    const int n_reg = bs.regions < kBucketMaxRegions ? bs.regions : kBucketMaxRegions;
    const int picks = bs.picks < kBucketPicks ? (bs.picks < n_reg ? bs.picks : n_reg) : (kBucketPicks < n_reg ? kBucketPicks : n_reg);
    // what needs nothing of the query is requested before it (two dependent scalar loads and a norm)
    Row cent[2];
    int2 tab[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = tid + u * kHalfSeedBlock;
        cent[u] = load_row(bs.centroids, static_cast<int64_t>(i < n_cent ? i : 0));
        tab[u] = bs.region_tab[i < n_reg ? i : 0];
    }
    float q[kDim];
    q8_load_query(query_ptr, by_value, q);
    const float qn = query_norm(q);
    const Q8Query hq = q8_query(q, qn);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = tid + u * kHalfSeedBlock;
        if (i < n_cent) s_cent[i] = score_to_ordered(cosine_score(q, qn, cent[u]));
    }
    if (tid < kBucketPicks) s_pick[tid] = -1;
    if (tid == 0) *s_count = 0;
    __syncthreads();
    uint32_t best_of[2];   // the region's best centroid score, ordered (0: no such region)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int g = tid + u * kHalfSeedBlock;
        best_of[u] = 0u;
        if (g < n_reg) {
            int first = tab[u].x < 0 ? 0 : (tab[u].x < n_cent ? tab[u].x : n_cent - 1);
            int last = tab[u].y < first ? first : (tab[u].y < n_cent ? tab[u].y : n_cent - 1);
            uint32_t m = 0u;
#pragma unroll
            for (int i = 0; i < kBucketSpanMax; ++i) {   // (independent reads, clamped to the range: all in flight at once)
                const uint32_t c = s_cent[first + i < last ? first + i : last];
                m = c > m ? c : m;
            }
            best_of[u] = m;
        }
    }
    // The regions to read: those whose score reaches the picks-th best score (handoff.hip.h, kth_of_values: one histogram
    // pass; ranking all pairs by counting was built first and cost the riders 14 us at 976 regions), the first `picks` of
    // them in region order — a block-wide prefix sum, the same in every rider.
    const float vth = kth_of_values<kHalfSeedBlock, 2>(best_of, n_reg, picks, s_count, sel, s_bins);
    const uint32_t need = vth > -__builtin_inff() ? score_to_ordered(vth) : 1u;   // (-inf: fewer scored regions than picks: all of them)
    const int chosen0 = best_of[0] != 0u && best_of[0] >= need, chosen1 = best_of[1] != 0u && best_of[1] >= need;
    const int incl = wave_inclusive_scan(chosen0 | (chosen1 << 16));
    __syncthreads();   // (kth_of_values is done with its scratch)
    if (lane == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kHalfSeedBlock / 64; ++w) {   // (uniform reads)
        const int t = s_wave[w];
        before += w < (tid >> 6) ? t : 0;
        total += t;
    }
    const int slot0 = ((before + incl) & 0xffff) - chosen0;
    const int slot1 = (total & 0xffff) + ((before + incl) >> 16) - chosen1;   // regions 512 .. 1023 come after regions 0 .. 511
    if (chosen0 && slot0 < picks) s_pick[slot0] = tid;
    if (chosen1 && slot1 < picks) s_pick[slot1] = tid + kHalfSeedBlock;
    __syncthreads();
    for (int k0 = rider; k0 < picks; k0 += kBucketAhead * n_wgs) {
        HalfTile t[kBucketAhead];
        bool live[kBucketAhead];
        int4 ids[kBucketAhead];
#pragma unroll
        for (int u = 0; u < kBucketAhead; ++u) {
            const int k = k0 + u * n_wgs;
            int g = s_pick[k < picks ? k : rider];
            live[u] = k < picks && g >= 0 && g < n_reg;   // uniform
            g = live[u] ? g : 0;
            const uint4* p = bs.q8 + (static_cast<int64_t>(g) * kHalfSeedBlock + tid) * 3;
            t[u].t0 = p[0];
            t[u].t1 = p[1];
            t[u].t2 = p[2];
            // (the lane's four row numbers ride along: looked up after the pick they would be one more dependent round trip)
            ids[u] = reinterpret_cast<const int4*>(bs.rows)[static_cast<int64_t>(g) * kHalfSeedBlock + tid];
        }
        int32_t idx[kBucketAhead];
        bool mine[kBucketAhead];
#pragma unroll
        for (int u = 0; u < kBucketAhead; ++u) {
            int a[4];
            bool special[4];
            q8_dot4(hq, t[u], a, special);
            uint32_t v = 0u;
            int best = 0;
            const int id4[4] = {ids[u].x, ids[u].y, ids[u].z, ids[u].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // (as q8_region_pick: padding, a row number outside the shard and the excluded row are left out BEFORE the
                // group's best is chosen, so such a group still yields its best eligible row)
                const bool use = hq.ok && !special[r] && id4[r] >= 0 && static_cast<int64_t>(id4[r]) < n &&
                                 row_base + id4[r] != exclude_global;
                const uint32_t w = use ? score_to_ordered(q8_approx(hq, a[r])) : 0u;
                best = w > v ? r : best;
                v = w > v ? w : v;
            }
            const uint32_t top = row16_max_u32(v);
            const uint64_t holders = __ballot(v == top && v != 0u);
            const uint32_t in_row = static_cast<uint32_t>(holders >> (lane & 48)) & 0xffffu;
            mine[u] = in_row != 0u && static_cast<int>(__builtin_ctz(in_row)) == (lane & 15);   // the row's first holder
            idx[u] = best == 0 ? id4[0] : (best == 1 ? id4[1] : (best == 2 ? id4[2] : id4[3]));
        }
        Row rows[kBucketAhead];
        bool ok[kBucketAhead];
#pragma unroll
        for (int u = 0; u < kBucketAhead; ++u) {
            ok[u] = mine[u] && idx[u] >= 0 && static_cast<int64_t>(idx[u]) < n && row_base + idx[u] != exclude_global;
            rows[u] = load_row(feats, ok[u] ? static_cast<int64_t>(idx[u]) : static_cast<int64_t>(0));
        }
#pragma unroll
        for (int u = 0; u < kBucketAhead; ++u) {
            const int k = k0 + u * n_wgs;
            const float exact = cosine_score(q, qn, rows[u]);
            // written THROUGH to device scope, under the query's epoch (q8_region_store)
            if (ok[u] && live[u] && !drop)
                __hip_atomic_store(&out[k * kBucketGroups + (tid >> 4)], tag_value(epoch, score_to_ordered(exact)), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return hq;
}

// One workgroup per region (single queries; the first query of a stream) and, when the grid has one more workgroup
// than regions, the neighbourhood of the excluded row (handoff.hip.h) by that last one.  `exact`: the sample values are
// EXACT scores (q8_region_store) — a kernel argument, not a template parameter: both kinds share one kernel.
__global__ __launch_bounds__(kHalfSeedBlock) void seed_q8_kernel(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int64_t stride_rows, int64_t row_base, QueryArg qarg,
    const float* __restrict__ query_ptr /* null: the query is qarg.q */, int64_t exclude_global,
    unsigned long long* __restrict__ seed_vals, uint32_t epoch, int regions, int topk,
    const float* __restrict__ anchors /* the handle's anchor table (handoff.hip.h), or null */, bool exact,
    BucketSample bucket /* rows != null: `regions` workgroups share the bucketed sample's regions instead */) {
    if (static_cast<int>(blockIdx.x) >= regions) {   // uniform
        // (1024 rows: this workgroup is the last one out of the sample launch of a query alone, and the scan subtracts a margin
        // of ~0.01 from whatever bound it is given — the 10th percentile of the neighbourhood serves it as well as the 5th)
        __shared__ int s_scratch[Nbhd<kHalfSeedBlock, 1024>::kScratch];
        nbhd_to_slot<kHalfSeedBlock, 1024>(feats, n, row_base, query_ptr, qarg.q, exclude_global, topk, epoch, seed_vals, s_scratch, anchors);
        return;
    }
    if (bucket.rows) {   // uniform
        __shared__ int s_bucket[kBucketScratch];
        __shared__ SelectSmem s_bucket_sel;
        (void)q8_bucket_sample(feats, bucket, n, row_base, query_ptr, qarg.q, exclude_global, seed_vals, epoch,
                               static_cast<int>(blockIdx.x), regions, false, s_bucket, s_bucket_sel);
        return;
    }
    // the region's rows are requested FIRST: they need nothing of the query, whose 12 floats sit behind two dependent
    // scalar loads and a norm (this launch is on the critical path of a query alone)
    const Q8Region s = q8_region_load(q8, (n + 3) >> 2, stride_rows, blockIdx.x);
    float q[kDim];
    q8_load_query(query_ptr, qarg.q, q);
    const float qn = query_norm(q);
    const Q8Query hq = q8_query(q, qn);
    const Q8Pick p = q8_region_pick(s, hq, n, row_base, exclude_global);
    Row row;
    row.a = row.b = row.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (exact) row = load_row(feats, p.row);   // (uniform)
    q8_region_store(p, row, q, qn, seed_vals, epoch, blockIdx.x, exact);
}

// The seed riders of a streamed launch (handoff.hip.h, NextSeed): four regions per memory round trip.
__device__ __forceinline__ Q8Query q8_seed_rider(const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n,
                                                 int64_t row_base, const NextSeed& next, int rider) {
    const int64_t n_quads = (n + 3) >> 2;
    unsigned long long* const out = static_cast<unsigned long long*>(next.out);
    constexpr int kAhead = 4;
    // A round's regions are requested before anything that does not need them: the first round before the QUERY is
    // (two dependent scalar loads and a norm: on a 1 M-row shard the riders' chain is the longest thing in the launch),
    // every later one right after the round before has been reduced, under its winners' fetches and stores.
    Q8Region s[kAhead];
    auto load_round = [&](int g0) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int g = g0 + u * next.n_wgs;
            s[u] = q8_region_load(q8, n_quads, next.stride_rows, g < next.regions ? g : rider);
        }
    };
    if (rider < next.regions) load_round(rider);
    float q[kDim];
    q8_load_query(next.query_ptr, next.q, q);
    const float qn = query_norm(q);
    const Q8Query hq = q8_query(q, qn);
    for (int g0 = rider; g0 < next.regions; g0 += kAhead * next.n_wgs) {
        Q8Pick pick[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) pick[u] = q8_region_pick(s[u], hq, n, row_base, next.exclude_global);
        if (g0 + kAhead * next.n_wgs < next.regions) load_round(g0 + kAhead * next.n_wgs);   // uniform
        if (next.exact) {   // uniform: the four winners' rows, one more round trip with four fetches in flight
            Row best[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) best[u] = load_row(feats, pick[u].row);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int g = g0 + u * next.n_wgs;
                if (g < next.regions && g >= next.debug_skip) q8_region_store(pick[u], best[u], q, qn, out, next.epoch, g, true);   // uniform
            }
        } else {
            Row none;
            none.a = none.b = none.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int g = g0 + u * next.n_wgs;
                if (g < next.regions && g >= next.debug_skip) q8_region_store(pick[u], none, q, qn, out, next.epoch, g, false);   // uniform
            }
        }
    }
    return hq;
}

// The launch-wide cutoff from n_seed sample values (handoff.hip.h: sample_kth_value): a row whose approximate score
// is below it cannot be among the best topk.  -inf when the sample cannot say, or the bound cannot be claimed for
// the query.  One margin below an EXACT score of a real row, two below an approximate one (the margin carries its
// own slack).
template <int kBlock>
__device__ __forceinline__ float q8_cutoff_from_sample(const Sample& sample, int n_seed, int topk, bool exact_values,
                                                       const Q8Query& hq, int* s_seeds /* zeroed */, SelectSmem& s_sel,
                                                       int* s_bins /* kSelScratch ints nobody else is using */) {
    if (!hq.ok) return -__builtin_inff();   // uniform
    const float v = sample_kth_value<kBlock>(sample, n_seed, topk, s_seeds, s_sel, s_bins);
    return exact_values ? v - hq.margin : v - 2.0f * hq.margin;   // (-inf stays -inf)
}

// ---- the workgroups of a streamed launch that do not scan (scan_q8_kernel, scan_q8_kernel_pair) --------------------------
// The merger of a query before: its per-workgroup lists into the caller's keys.
template <typename MergeSmem>
__device__ __forceinline__ void q8_ride_merge(MergeSmem& sm, const PrevMerge& prev) {
    if (prev.lists)
        merge_body(sm, prev.lists, prev.n_lists, prev.topk, static_cast<int64_t>(prev.topk), static_cast<int64_t>(0), prev.topk,
                   prev.out_keys, static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr), static_cast<int64_t>(0),
                   static_cast<int64_t>(0), static_cast<int64_t>(0));
}

// The neighbourhood of a query after (handoff.hip.h): read by the launch that scans for it.
template <int kBlock>
__device__ __forceinline__ void q8_ride_nbhd(const float* __restrict__ feats, int64_t n, int64_t row_base, const NextSeed& next,
                                             int* s_scratch) {
    nbhd_to_slot<kBlock>(feats, n, row_base, next.query_ptr, next.q, next.exclude_global, next.topk, next.epoch,
                         static_cast<unsigned long long*>(next.out), s_scratch, next.anchors);
}

// Seed rider `rider` of next.n_wgs: its share of the sample of a query after, strided or bucketed.  s_scratch: kBucketScratch
// ints of LDS nobody else is using.
template <int kBlock>
__device__ __forceinline__ void q8_ride_sample(const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int64_t row_base,
                                               const NextSeed& next, int rider, int* s_scratch, int* s_flag, int* s_seeds,
                                               SelectSmem& s_sel) {
    const bool bucketed = next.bucket.rows != nullptr;   // uniform
    // (DROP_STORES, the test hook: the bucketed riders drop every store)
    const Q8Query nq = bucketed ? q8_bucket_sample(feats, next.bucket, n, row_base, next.query_ptr, next.q, next.exclude_global,
                                                   static_cast<unsigned long long*>(next.out), next.epoch, rider, next.n_wgs,
                                                   next.debug_skip > 0, s_scratch, s_sel)
                                : q8_seed_rider(feats, q8, n, row_base, next, rider);
    const int n_vals = bucketed ? kBucketPicks * kBucketGroups : next.regions * kHalfSeedWaves;
    // Last rider out turns the sample into the cutoff (handoff.hip.h, sample_arrive_and_select: no device-wide
    // fence under the scanners).  Values and cutoff carry the next query's epoch and the counter is never reset.
    if (next.ctl) {   // uniform; null: nobody reads the sample inside this launch (small shards: the next launch selects)
        float v;
        if (sample_arrive_and_select<kBlock>(next.ctl, next.done_base, static_cast<unsigned>(next.n_wgs),
                                             static_cast<const unsigned long long*>(next.out), n_vals, next.topk, next.epoch, s_flag,
                                             s_seeds, s_sel, s_scratch, v)) {
            // one margin below an EXACT score of a real row, two below an approximate one
            const float c = !nq.ok ? -__builtin_inff() : (next.exact != 0 ? v - nq.margin : v - 2.0f * nq.margin);
            if (threadIdx.x == 0) next.ctl->cutoff = tag_value(next.epoch, __float_as_uint(c));
        }
    }
}

// ---- the scan ----------------------------------------------------------------------------------------------
template <int kBlockT, int kMinWavesT, int kDepthT>
struct Q8Cfg {
    static constexpr int kBlock = kBlockT;
    static constexpr int kMinWaves = kMinWavesT;
    static constexpr int kDepth = kDepthT;
    static constexpr int kTileRows = 4 * kBlockT;
    static constexpr int kCandCap = kCandLimit + kTileRows;
    static constexpr int kCandPerThread = (kCandCap + kBlockT - 1) / kBlockT;
};
using DefaultQ8Cfg = Q8Cfg<512, 4, 2>;

// kWithMerge (streamed queries): workgroups [0, S) scan, workgroup S merges the PREVIOUS streamed query, the next
// next.n_wgs workgroups are seed riders for the NEXT one and (next.nbhd) the last of the grid takes that query's
// neighbourhood (handoff.hip.h); S = gridDim.x - 1 - next.n_wgs - next.nbhd.  Those are the roles' VIRTUAL ids (`vb`): in
// hardware the 1 + n_wgs + nbhd workgroups that do not scan hold the FIRST block ids, so that they are dispatched first.
// Slot kNbhdSlot of `seed_vals` holds, under this query's epoch, the neighbourhood's EXACT bound v (0: none): keys below
// it are dropped at once and v - margin is one more lower bound on the cutoff — what keeps a catalogue sorted by genre
// (the query's cluster in ONE sampled region at most) from scanning with another cluster's cutoff.
//
// Tiles are dealt round-robin.  Handing them out dynamically (ticket counters, the merger and the riders joining
// once their job was done) was built and measured: every workgroup then finished within 2 us of the others
// instead of 8 — and the launch took as long as before, because between prologue and last tile the launch
// already moves its bytes at ~6.5 TB/s and early finishers only leave that bandwidth to the rest.
//
// kLoneTail (a lone query whose caller waits on the host): the workgroup that finishes last merges the lists of
// THIS launch into the caller's buffers and raises the completion word (kernels.hip.h, lone_tail).
//
// kQueryFromRow is a compile-time choice for the plain and the lone-tail forms only.  The STREAMED form exists once
// (<Cfg, false, true>) and takes the run-time test q8_load_query makes anyway — query_ptr, or qarg.q where that is
// null: its kernel slot went to scan_q8_kernel_pair (the library's kernel count is capped).
template <typename Cfg, bool kQueryFromRow, bool kWithMerge, bool kLoneTail = false>
__global__ __launch_bounds__(Cfg::kBlock, Cfg::kMinWaves) void scan_q8_kernel(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int iters, int64_t row_base,
    QueryArg qarg, const float* __restrict__ query_ptr, int64_t exclude_global, int topk, uint64_t* __restrict__ block_lists,
    const unsigned long long* __restrict__ seed_vals /* tagged with `epoch` */, int n_seed /* negative: |n_seed| EXACT sample values */,
    unsigned long long* __restrict__ rescored /* [scanning workgroups] */,
    PrevMerge prev, NextSeed next, const unsigned long long* __restrict__ cutoff_ready /* tagged; null: select from seed_vals here */,
    LoneTail lone, uint32_t epoch /* of this query */) {
    constexpr int kBlock = Cfg::kBlock;
    static_assert(!(kWithMerge && kLoneTail), "a streamed query's merge rides in the next launch");
    __shared__ typename std::conditional<kWithMerge || kLoneTail, HalfScanOrMergeSmem<Cfg>, HalfScanSmemT<Cfg>>::type s_mem;
    __shared__ int s_lone_flag;
    HalfScanSmemT<Cfg>* sm;
    unsigned nblocks = gridDim.x;   // scanning workgroups
    unsigned vb = blockIdx.x;       // this workgroup's place among them (and, kWithMerge, behind them: see below)
    MI355REC_PHASE(0);
    if constexpr (kWithMerge) {
        // The workgroups that do not scan take the FIRST block ids — they are dispatched first: at the end of the grid they
        // only got their slots once workgroups of the launch before had finished, and a rider's chain of dependent round
        // trips, started that late, was the last thing to finish in the launch.  `vb` is the id every role is told by.
        const unsigned extra = 1u + static_cast<unsigned>(next.n_wgs) + static_cast<unsigned>(next.nbhd);
        nblocks = gridDim.x - extra;
        vb = blockIdx.x >= extra ? blockIdx.x - extra : nblocks + blockIdx.x;
        if (vb >= nblocks) {
            if (vb == nblocks) {
                q8_ride_merge(s_mem.merge, prev);
            } else if (next.nbhd && vb == gridDim.x - 1u) {   // the next query's neighbourhood: read by the NEXT launch
                q8_ride_nbhd<kBlock>(feats, n, row_base, next, reinterpret_cast<int*>(s_mem.scan.cand));
            } else {
                static_assert(kBlock == kHalfSeedBlock && sizeof(s_mem.scan.cand) >= sizeof(int) * kBucketScratch, "the riders' geometry");
                q8_ride_sample<kBlock>(feats, q8, n, row_base, next, static_cast<int>(vb - nblocks - 1u), reinterpret_cast<int*>(s_mem.scan.cand),
                                       &s_mem.scan.count, &s_mem.scan.seeds, s_mem.scan.sel);
            }
            __syncthreads();
            MI355REC_PHASE(5);
            return;
        }
        sm = &s_mem.scan;
    } else if constexpr (kLoneTail) {
        (void)next;
        sm = &s_mem.scan;
    } else {
        (void)next;
        (void)lone;
        (void)s_lone_flag;
        sm = &s_mem;
    }
    uint64_t* const s_cand = sm->cand;
    SelectSmem& s_sel = sm->sel;
    int& s_count = sm->count;

    const unsigned bid = vb;
    const int tid = threadIdx.x;
    const int lane = tid & 63;

    const int64_t n_quads = (n + 3) >> 2;
    const int64_t last_quad = n_quads - 1;
    const int64_t quad_begin = static_cast<int64_t>(bid) * kBlock + tid;
    const int64_t quad_stride = static_cast<int64_t>(nblocks) * kBlock;

    auto load_tile = [&](HalfTile& dst, int it) {
        int64_t quad = quad_begin + static_cast<int64_t>(it) * quad_stride;
        quad = quad < n_quads ? quad : last_quad;   // unconditional prefetch (see scan_kernel)
        const uint4* p = q8 + quad * 3;
        dst.t0 = p[0];
        dst.t1 = p[1];
        dst.t2 = p[2];
    };

    // everything the first tile needs is asked for at once: the finished cutoff — or, where this workgroup selects it
    // itself, the sample values, FIRST: they come back before the tile does and the selection runs under its latency —
    // the tile's 48 B per lane, the query
    constexpr int kDepth = Cfg::kDepth;
    float cutoff_left = 0.0f;
    const unsigned long long nbhd_raw = seed_vals[kNbhdSlot];   // (wave-uniform: a scalar load)
    SampleRaw sample_raw;
#pragma unroll
    for (int r = 0; r < kHalfSeedPerThread; ++r) sample_raw.t[r] = 0ull;
    const int n_sample = n_seed < 0 ? -n_seed : n_seed;
    if (cutoff_ready) {   // uniform: the riders of the launch before this one left it (under this query's epoch, or it does not count)
        cutoff_left = untag_cutoff(*cutoff_ready, epoch);
    } else {              // ... or this workgroup selects it from the sample values itself
        sample_raw = sample_request<kBlock>(seed_vals, n_sample);
    }
    HalfTile ring[kDepth];
#pragma unroll
    for (int d = 0; d < kDepth - 1; ++d) load_tile(ring[d], d);
    float q[kDim];
    q8_load_query((kQueryFromRow || kWithMerge) ? query_ptr : nullptr, qarg.q, q);
    const float qn = query_norm(q);
    const Q8Query hq = q8_query(q, qn);
    const Sample sample = sample_finish(sample_raw, epoch);
    if (hq.hi[0] != 0 || n >= 0) MI355REC_PHASE(1);   // (depends on the query: not hoisted above its load)
    if (sample.v[0] != 0x12345u || n >= 0) MI355REC_PHASE(6);   // (depends on this thread's sample values: they have arrived)

    // ---- launch-wide cutoff (while the first tiles are in flight)
    if (tid == 0) {
        s_count = 0;
        sm->seeds = 0;
        sm->rescored = 0;
    }
    int n_rescored = 0;   // wave-uniform: rows this wave sent to the exact chain (diagnostics)
    __syncthreads();
    float cutoff;
    if (cutoff_ready) {   // uniform
        cutoff = cutoff_left;
    } else {
        cutoff = q8_cutoff_from_sample<kBlock>(sample, n_sample, topk, n_seed < 0, hq, &sm->seeds, s_sel, reinterpret_cast<int*>(s_cand));
    }
    uint64_t thr = 0;
    if (const uint32_t nbv = untag_value(nbhd_raw, epoch)) {   // uniform: at least topk rows score >= this EXACT bound
        thr = (static_cast<uint64_t>(nbv) << 32) - 1ull;   // (a key AT the bound passes: key > thr)
        if (hq.ok) {
            const float nb_cut = ordered_to_score(nbv) - hq.margin;
            cutoff = nb_cut > cutoff ? nb_cut : cutoff;
        }
    }
    int cut_d = q8_threshold(cutoff);   // the cutoff's integer image: a row is out iff D < cut_d
    MI355REC_PHASE(2);
    int compact_at = 2 * topk > 256 ? 2 * topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;

    // A row the replica cannot rule out costs one random 48 B fetch from the fp32 matrix, ISSUED when the
    // row is found and CONSUMED one tile later (a one-entry pending slot per lane), so its latency overlaps
    // the next tile.  A lane's second, third and fourth candidate of one tile are scored on the spot (rare).
    Row pend;
    pend.a = pend.b = pend.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int64_t pend_r = 0;
    bool pend_on = false;

    auto append = [&](bool have, const Row& row, int64_t r) {
        const float s = cosine_score(q, qn, row);
        const int64_t g = row_base + r;
        uint64_t key = pack_key(s, static_cast<uint32_t>(g));
        if (g == exclude_global) key = 0;
        const bool pass = have && key > thr;
        const uint64_t ballot = __ballot(pass);
        if (ballot) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_count, __popcll(ballot));
            base = __builtin_amdgcn_readfirstlane(base);
            const int pos = base + lanes_below(ballot);
            if (pass) s_cand[pos] = key;
        }
    };
    auto consume = [&]() {
        if (__ballot(pend_on)) append(pend_on, pend, pend_r);
        pend_on = false;
    };

    auto process_tile = [&](const HalfTile& t, int it) {
        const int64_t quad = quad_begin + static_cast<int64_t>(it) * quad_stride;
        const int64_t r0 = quad * 4;
        int a[4];
        bool special[4];
        q8_dot4(hq, t, a, special);
        // The common case — no lane of the wave holds a candidate — is decided on the scalar side: four integer compares and four
        // byte compares per lane, their wave masks OR-ed.  Whether a row lies inside the shard at all (the last quad's
        // padding, the clamped prefetch past the end) only matters once something hit, and is settled there.
        bool hit[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) hit[u] = special[u] | (a[u] >= cut_d);
        const uint64_t maybe = __ballot(hit[0] | hit[1] | hit[2] | hit[3]);
        consume();   // the rows fetched while the previous tile was scanned
        uint32_t mask = 0u;   // which of the lane's four rows are candidates
        if (maybe) {          // uniform
            const int64_t left = n - r0;
            const int valid = quad < n_quads ? (left < 4 ? static_cast<int>(left) : 4) : 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) mask |= (hit[u] && u < valid) ? (1u << u) : 0u;
        }
        const uint64_t any = maybe ? __ballot(mask != 0u) : 0ull;
        if (any) {
            n_rescored += __popcll(any);
            const int first = mask ? __builtin_ctz(mask) : 0;
            // lanes without a candidate re-read row 0: one cached line
            pend_r = r0 + first;
            pend = load_row(feats, mask ? pend_r : static_cast<int64_t>(0));
            pend_on = mask != 0u;
            uint32_t rest = mask & (mask - 1u);   // the lane's further candidates, if any
            while (__ballot(rest != 0u)) {         // uniform, rare
                const int u = rest ? __builtin_ctz(rest) : 0;
                const bool have = rest != 0u;
                n_rescored += __popcll(__ballot(have));
                const Row extra = load_row(feats, have ? r0 + u : static_cast<int64_t>(0));
                append(have, extra, r0 + u);
                rest &= rest - 1u;
            }
        }
        __syncthreads();
        const int c = s_count;
        __syncthreads();
        if (c >= compact_at) {
            const uint64_t local_thr = compact_candidates<kBlock, Cfg::kCandPerThread>(s_cand, &s_count, topk, false, s_sel);
            if (local_thr > thr) {
                thr = local_thr;
                if (hq.ok) {
                    const float local_cut = ordered_to_score(static_cast<uint32_t>(thr >> 32)) - hq.margin;
                    cutoff = local_cut > cutoff ? local_cut : cutoff;
                    cut_d = q8_threshold(cutoff);
                }
            }
        }
    };

    for (int it = 0; it < iters; it += kDepth) {
#pragma unroll
        for (int sidx = 0; sidx < kDepth; ++sidx) {
            load_tile(ring[(sidx + kDepth - 1) % kDepth], it + sidx + kDepth - 1);
            if (it + sidx < iters) process_tile(ring[sidx], it + sidx);  // uniform
        }
    }
    consume();   // the last tile's fetches

    if (lane == 0 && n_rescored) atomicAdd(&sm->rescored, n_rescored);
    __syncthreads();
    MI355REC_PHASE(3);
    if (tid == 0) rescored[bid] += static_cast<unsigned long long>(sm->rescored);   // launches of a handle are stream-ordered
    // (from kRankCountMax keys up the ranking is a bitonic sort of the next power of two — 45 barrier stages, ~2.7 us
    // for the ~250 keys a scan without a launch-wide cutoff ends with; an INEXACT cut to topk + topk / 4 first costs a
    // radix pass or two and leaves a set the counting rank handles)
    if (s_count > kRankCountMax && s_count > topk)  // uniform
        compact_candidates<kBlock, Cfg::kCandPerThread>(s_cand, &s_count, topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kBlock, kLoneTail>(s_cand, s_count, block_lists + static_cast<int64_t>(bid) * topk, topk);
    if constexpr (kLoneTail) lone_tail(s_mem.merge, &s_lone_flag, block_lists, topk, lone);
    __syncthreads();
    MI355REC_PHASE(4);
}

// ---- the scan for a PAIR of streamed queries -------------------------------------------------------------------------
// Two streamed queries queued on a handle each stream the same replica: 120 MB at 10 M rows, against ~50 vector
// instructions per lane and tile of work.  The pair form is scan_q8_kernel<.., kWithMerge> with TWO queries: a tile is
// loaded once and q8_dot4 runs against query A and then query B over the same registers.  Everything a query owns it
// owns here as well — cutoff, cut_d and thr, the candidate list in LDS and its compaction, the rescored count, the
// per-workgroup output list (the pending fetch slot alone is shared) — and everything after a hit (cosine_score, pack_key,
// block_rank_and_store) is the single form's, so the keys are the single form's bit for bit.  Both queries ask for the same topk <= kPairMaxTopk: the
// candidate lists are a quarter of the single form's (compaction starts at max(2 topk, 256) = 256 keys either way).
//
// Workgroups, by virtual id: [0, S) scan; the next Q = side.queries (2 or 4) merge the lists of the queries BEFORE
// (prev[0 .. Q)); then Q x next[0].n_wgs seed riders and Q x next[0].nbhd neighbourhood workgroups for the queries AFTER, each
// with its own sample buffer, SeedCtl and epoch.  As in the single form they hold the FIRST block ids.
constexpr int kPairMaxTopk = 128;

// A wave-uniform value the compiler holds in a vector register (whatever float arithmetic or an LDS read produced it), moved
// to a scalar one: two queries' digits, norms, cutoffs and thresholds are two dozen registers per lane otherwise.
__device__ __forceinline__ int q8_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float q8_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ uint64_t q8_uniform(uint64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v))));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v >> 32))));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ Q8Query q8_uniform(const Q8Query& q) {
    Q8Query r;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r.hi[j] = q8_uniform(q.hi[j]);
        r.lo[j] = q8_uniform(q.lo[j]);
    }
    r.inv = q.inv;
    r.margin = q8_uniform(q.margin);
    r.ok = q8_uniform(q.ok ? 1 : 0) != 0;
    return r;
}
constexpr int kPairCandLimit = 2 * kPairMaxTopk;   // a tile is never entered with more candidates of one query

// The pair kernel's tile loop is bound by vector issue (docs/LAB_NOTES.md, "Streamed 8-bit scan: fewer vector instructions per
// tile in the pair kernel"), and all it asks of a row's D is whether it reaches the query's cut_d.  So it computes the EXCESS
// D - cut_d in one accumulator chain, eight instructions a row where q8_dot and its compare take ten: the low digits' chain
// starts from 256 * hi - cut_d (one v_lshl_add_u32) instead of from a cleared register, and nothing is compared per row.  The
// same integer sums as q8_dot: a row is a candidate where the excess is >= 0.  `neg_cut` is -cut_d, kept per query beside
// cut_d; a cut of INT_MIN ("no bound") is clamped to -2^30, which no D comes near (|D| < 2^27).  (Plain builtins on purpose:
// the dot instructions have issue hazards against other vector instructions on this chip that the compiler pads for, and it
// cannot see into inline assembly.)
__device__ __forceinline__ int q8_pair_neg_cut(int cut_d) { return -(cut_d > -(1 << 30) ? cut_d : -(1 << 30)); }
__device__ __forceinline__ int q8_pair_excess(const Q8Query& q, int neg_cut, uint32_t d0, uint32_t d1, uint32_t d2) {
    int hi = __builtin_amdgcn_sdot4(static_cast<int>(d0), q.hi[0], 0, false);
    hi = __builtin_amdgcn_sdot4(static_cast<int>(d1), q.hi[1], hi, false);
    hi = __builtin_amdgcn_sdot4(static_cast<int>(d2), q.hi[2], hi, false);
    if constexpr (kQ8QueryBits == 16) {
        int acc = static_cast<int>((static_cast<uint32_t>(hi) << 8) + static_cast<uint32_t>(neg_cut));
        acc = __builtin_amdgcn_sdot4(static_cast<int>(d0), q.lo[0], acc, false);
        acc = __builtin_amdgcn_sdot4(static_cast<int>(d1), q.lo[1], acc, false);
        acc = __builtin_amdgcn_sdot4(static_cast<int>(d2), q.lo[2], acc, false);
        return acc;
    } else {
        return hi + neg_cut;
    }
}
__device__ __forceinline__ void q8_pair_excess4(const Q8Query& q, int neg_cut, const HalfTile& t, int (&e)[4]) {
    e[0] = q8_pair_excess(q, neg_cut, t.t0.x, t.t0.y, t.t0.z);
    e[1] = q8_pair_excess(q, neg_cut, t.t0.w, t.t1.x, t.t1.y);
    e[2] = q8_pair_excess(q, neg_cut, t.t1.z, t.t1.w, t.t2.x);
    e[3] = q8_pair_excess(q, neg_cut, t.t2.y, t.t2.z, t.t2.w);
}

template <int kBlockT, int kMinWavesT, int kDepthT>
struct Q8PairCfg {
    static constexpr int kBlock = kBlockT;
    static constexpr int kMinWaves = kMinWavesT;
    static constexpr int kDepth = kDepthT;
    static constexpr int kTileRows = 4 * kBlockT;
    static constexpr int kCandCap = kPairCandLimit + kTileRows;
    static constexpr int kCandPerThread = (kCandCap + kBlockT - 1) / kBlockT;
};
using DefaultQ8PairCfg = Q8PairCfg<512, 4, 2>;

template <typename Cfg>
struct Q8PairSmemT {
    uint64_t cand[2][Cfg::kCandCap];
    SelectSmem sel;   // (the two queries select one after the other)
    int count[2];
    int seeds[2];
    int rescored;
};
template <typename Cfg>
union Q8PairOrMergeSmem {
    Q8PairSmemT<Cfg> scan;
    MergeSmemT<Cfg::kBlock, kRideMaxLists, kHalfRideSurvCap> merge;
};

// One query of a pair launch: what scan_q8_kernel takes as separate arguments.
struct Q8PairArg {
    QueryArg qarg;
    const float* query_ptr;                       // null: the query is qarg.q
    long long exclude_global;
    uint64_t* block_lists;                        // [scanning workgroups][topk]
    const unsigned long long* seed_vals;          // tagged with `epoch`
    const unsigned long long* cutoff_ready;       // tagged; null: select from seed_vals here
    int n_seed;                                   // negative: |n_seed| EXACT sample values
    uint32_t epoch;
};

// What the workgroups of a launch that do not scan are given: indexed by a run-time (uniform) index, so that every role
// exists once in the kernel's code and reads the arguments of ITS query from the kernel's argument block.  `queries` is 2 or
// 4: that many mergers, and that many queries after with `riders` seed riders and `nbhd` neighbourhood workgroups each (a
// query slot nobody filled — prev.lists or next.out null — costs its workgroups an early return).
struct Q8PairSide {
    PrevMerge prev[4];   // the lists of the pair (or the two pairs) before
    NextSeed next[4];    // the queries of the pair (or the two pairs) after: the same n_wgs and nbhd in all
    int queries;
    int pad;
};

// The queries a launch scans for: pair g is q[2g], q[2g + 1].  A scanning workgroup picks its pair by a uniform run-time
// index into the kernel's argument block, as the other roles pick theirs from Q8PairSide.
struct Q8PairArgs {
    Q8PairArg q[4];
};

// TWO PAIRS PER LAUNCH (pairs == 2).  The scanners split into two halves of H = S / 2, one per pair; every tile slot j < H is
// scanned by two workgroups, one per pair ("twins").  Where H >= 8 (the host keeps it a multiple of 8 then) scanner s serves
// pair (s >> 3) & 1 and slot ((s >> 4) << 3) | (s & 7): twins are scanners s and s ^ 8, whose block ids lie exactly 8 apart —
// on the hardware this was written for they land on the same XCD at nearly the same time, so that the tile one of them
// fetches is found in that XCD's L2 by the other.  Nothing but speed depends on that: no workgroup waits for another, and a
// twin that runs alone or late computes the same keys.  A query's lists are block_lists[j], H of them; `rescored` stays per
// scanning workgroup.  pairs == 1: H = S, slot = s — the launch of one pair as it always was.
template <typename Cfg>
__global__ __launch_bounds__(Cfg::kBlock, Cfg::kMinWaves) void scan_q8_kernel_pair(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int iters, int64_t row_base, Q8PairArgs args,
    int pairs /* 1 or 2 */, int topk, unsigned long long* __restrict__ rescored /* [scanning workgroups] */, Q8PairSide side) {
    constexpr int kBlock = Cfg::kBlock;
    __shared__ Q8PairOrMergeSmem<Cfg> s_mem;
    const unsigned riders = static_cast<unsigned>(side.next[0].n_wgs), nbhds = static_cast<unsigned>(side.next[0].nbhd);
    const unsigned nq = static_cast<unsigned>(side.queries);
    const unsigned extra = nq * (1u + riders + nbhds);
    const unsigned nblocks = gridDim.x - extra;   // scanning workgroups
    const unsigned vb = blockIdx.x >= extra ? blockIdx.x - extra : nblocks + blockIdx.x;
    if (vb >= nblocks) {
        static_assert(kBlock == kHalfSeedBlock && sizeof(s_mem.scan.cand) >= sizeof(int) * kBucketScratch &&
                          sizeof(s_mem.scan.cand) >= sizeof(int) * Nbhd<kBlock>::kScratch, "the riders' geometry");
        int* const s_scratch = reinterpret_cast<int*>(s_mem.scan.cand);
        const unsigned e = vb - nblocks;   // uniform
        if (e < nq) {
            q8_ride_merge(s_mem.merge, side.prev[e]);
        } else if (e < nq + nq * riders) {
            const unsigned which = (e - nq) / riders;
            if (side.next[which].out)
                q8_ride_sample<kBlock>(feats, q8, n, row_base, side.next[which], static_cast<int>(e - nq - which * riders), s_scratch,
                                       &s_mem.scan.count[0], &s_mem.scan.seeds[0], s_mem.scan.sel);
        } else {
            const unsigned which = e - nq - nq * riders;
            if (side.next[which].out) q8_ride_nbhd<kBlock>(feats, n, row_base, side.next[which], s_scratch);
        }
        __syncthreads();
        return;
    }
    Q8PairSmemT<Cfg>* const sm = &s_mem.scan;
    SelectSmem& s_sel = sm->sel;

    // which pair this workgroup scans for, and which tile slot of that pair's `slots` it is (uniform)
    unsigned group = 0u, bid = vb, slots = nblocks;
    if (pairs == 2) {
        slots = nblocks >> 1;
        if (slots >= 8u) {
            group = (vb >> 3) & 1u;
            bid = ((vb >> 4) << 3) | (vb & 7u);
        } else {   // (tiny shards: any mapping that gives each pair `slots` slots)
            group = vb >= slots ? 1u : 0u;
            bid = vb - group * slots;
        }
    }
    const Q8PairArg& arg_a = args.q[2u * group];
    const Q8PairArg& arg_b = args.q[2u * group + 1u];
    const int tid = threadIdx.x;
    const int lane = tid & 63;

    const int64_t n_quads = (n + 3) >> 2;
    const int64_t last_quad = n_quads - 1;
    const int64_t quad_begin = static_cast<int64_t>(bid) * kBlock + tid;
    const int64_t quad_stride = static_cast<int64_t>(slots) * kBlock;

    // Tiles are asked for in order (it = 0, 1, 2, ...), so where the lane's next one starts (counted in uint4s) is where the last
    // one did plus a uniform stride: five vector instructions a tile where quad_begin + it * quad_stride, the clamp and "times
    // 48 plus the base" take ten.  The count runs on past the end and is clamped to the last quad's when it is used.
    const int64_t last_at = last_quad * 3;
    const int64_t stride_at = quad_stride * 3;
    int64_t next_at = quad_begin * 3;
    auto load_tile = [&](HalfTile& dst, int /* it: the next one */) {
        const uint4* p = q8 + (next_at < last_at ? next_at : last_at);   // unconditional prefetch (see scan_kernel)
        next_at += stride_at;
        dst.t0 = p[0];
        dst.t1 = p[1];
        dst.t2 = p[2];
    };

    // What one query of the pair owns (scan_q8_kernel's locals).
    struct Mine {
        float q[kDim];
        float qn;
        Q8Query hq;
        float cutoff;
        uint64_t thr;
        int cut_d;
        int neg_cut;      // -cut_d for q8_pair_excess, kept in step with cut_d
        int n_rescored;   // wave-uniform
        uint64_t* s_cand;
        int* s_count;
    };
    Mine A, B;
    A.s_cand = sm->cand[0];
    B.s_cand = sm->cand[1];
    A.s_count = &sm->count[0];
    B.s_count = &sm->count[1];

    // as the single form: the finished cutoffs — or the sample values — are asked for first, then the tile, then the queries
    constexpr int kDepth = Cfg::kDepth;
    const unsigned long long nbhd_raw_a = arg_a.seed_vals[kNbhdSlot], nbhd_raw_b = arg_b.seed_vals[kNbhdSlot];   // (scalar loads)
    float left_a = 0.0f, left_b = 0.0f;
    SampleRaw raw_a, raw_b;
#pragma unroll
    for (int r = 0; r < kHalfSeedPerThread; ++r) raw_a.t[r] = raw_b.t[r] = 0ull;
    const int n_sample_a = arg_a.n_seed < 0 ? -arg_a.n_seed : arg_a.n_seed, n_sample_b = arg_b.n_seed < 0 ? -arg_b.n_seed : arg_b.n_seed;
    if (arg_a.cutoff_ready) left_a = untag_cutoff(*arg_a.cutoff_ready, arg_a.epoch);   // uniform
    else raw_a = sample_request<kBlock>(arg_a.seed_vals, n_sample_a);
    if (arg_b.cutoff_ready) left_b = untag_cutoff(*arg_b.cutoff_ready, arg_b.epoch);   // uniform
    else raw_b = sample_request<kBlock>(arg_b.seed_vals, n_sample_b);
    HalfTile ring[kDepth];
#pragma unroll
    for (int d = 0; d < kDepth - 1; ++d) load_tile(ring[d], d);
    q8_load_query(arg_a.query_ptr, arg_a.qarg.q, A.q);
    q8_load_query(arg_b.query_ptr, arg_b.qarg.q, B.q);
    A.qn = q8_uniform(query_norm(A.q));
    B.qn = q8_uniform(query_norm(B.q));
    A.hq = q8_uniform(q8_query(A.q, A.qn));
    B.hq = q8_uniform(q8_query(B.q, B.qn));

    if (tid == 0) {
        sm->count[0] = sm->count[1] = 0;
        sm->seeds[0] = sm->seeds[1] = 0;
        sm->rescored = 0;
    }
    __syncthreads();
    // ---- the launch-wide cutoffs (while the first tiles are in flight), one query after the other
    auto start = [&](Mine& m, const Q8PairArg& arg, const SampleRaw& raw, int n_sample, float left, unsigned long long nbhd_raw, int* s_seeds) {
        if (arg.cutoff_ready) {   // uniform
            m.cutoff = left;
        } else {
            const Sample sample = sample_finish(raw, arg.epoch);
            m.cutoff = q8_cutoff_from_sample<kBlock>(sample, n_sample, topk, arg.n_seed < 0, m.hq, s_seeds, s_sel, reinterpret_cast<int*>(m.s_cand));
        }
        m.thr = 0;
        if (const uint32_t nbv = untag_value(nbhd_raw, arg.epoch)) {   // uniform: at least topk rows score >= this EXACT bound
            m.thr = (static_cast<uint64_t>(nbv) << 32) - 1ull;         // (a key AT the bound passes: key > thr)
            if (m.hq.ok) {
                const float nb_cut = ordered_to_score(nbv) - m.hq.margin;
                m.cutoff = nb_cut > m.cutoff ? nb_cut : m.cutoff;
            }
        }
        m.cutoff = q8_uniform(m.cutoff);
        m.thr = q8_uniform(m.thr);
        m.cut_d = q8_uniform(q8_threshold(m.cutoff));
        m.neg_cut = q8_uniform(q8_pair_neg_cut(m.cut_d));
        m.n_rescored = 0;
    };
    start(A, arg_a, raw_a, n_sample_a, left_a, nbhd_raw_a, &sm->seeds[0]);
    __syncthreads();   // (B's selection shares s_sel with A's)
    start(B, arg_b, raw_b, n_sample_b, left_b, nbhd_raw_b, &sm->seeds[1]);
    int compact_at = 2 * topk > 256 ? 2 * topk : 256;
    if (compact_at > kPairCandLimit) compact_at = kPairCandLimit;

    auto append = [&](Mine& m, int64_t exclude_global, bool have, const Row& row, int64_t r) {
        const float s = cosine_score(m.q, m.qn, row);
        const int64_t g = row_base + r;
        uint64_t key = pack_key(s, static_cast<uint32_t>(g));
        if (g == exclude_global) key = 0;
        const bool pass = have && key > m.thr;
        const uint64_t ballot = __ballot(pass);
        if (ballot) {
            int base = 0;
            if (lane == 0) base = atomicAdd(m.s_count, __popcll(ballot));
            base = __builtin_amdgcn_readfirstlane(base);
            const int pos = base + lanes_below(ballot);
            if (pass) m.s_cand[pos] = key;
        }
    };
    // The pending fetch slot (scan_q8_kernel: issued when a candidate row is found, consumed one tile later) is SHARED: one
    // row per lane, with a bit per query it is a candidate of — a row both queries cannot rule out is fetched once.  A lane's
    // further candidate rows of the tile, of either query, are scored on the spot (rare).
    Row pend;
    pend.a = pend.b = pend.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int64_t pend_r = 0;
    uint32_t pend_for = 0u;   // bit 0: query A, bit 1: query B
    auto score_row = [&](uint32_t who, const Row& row, int64_t r) {
        if (__ballot((who & 1u) != 0u)) append(A, arg_a.exclude_global, (who & 1u) != 0u, row, r);
        if (__ballot((who & 2u) != 0u)) append(B, arg_b.exclude_global, (who & 2u) != 0u, row, r);
    };
    auto consume = [&]() {
        if (__ballot(pend_for != 0u)) score_row(pend_for, pend, pend_r);
        pend_for = 0u;
    };
    auto fetch = [&](uint32_t mask_a, uint32_t mask_b, int64_t r0) {
        const uint32_t both = mask_a | mask_b;
        if (!__ballot(both != 0u)) return;   // uniform
        auto whose = [&](int u) { return ((mask_a >> u) & 1u) | (((mask_b >> u) & 1u) << 1); };
        // (the books stay per query: every row a query sends to the exact chain counts for that query)
        auto count = [&](uint32_t who) {
            A.n_rescored += __popcll(__ballot((who & 1u) != 0u));
            B.n_rescored += __popcll(__ballot((who & 2u) != 0u));
        };
        const int first = both ? __builtin_ctz(both) : 0;
        pend_r = r0 + first;
        pend = load_row(feats, both ? pend_r : static_cast<int64_t>(0));   // (lanes without a candidate re-read row 0: one cached line)
        pend_for = both ? whose(first) : 0u;
        count(pend_for);
        uint32_t rest = both & (both - 1u);
        while (__ballot(rest != 0u)) {   // uniform, rare
            const int u = rest ? __builtin_ctz(rest) : 0;
            const uint32_t who = rest ? whose(u) : 0u;
            count(who);
            const Row extra = load_row(feats, rest ? r0 + u : static_cast<int64_t>(0));
            score_row(who, extra, r0 + u);
            rest &= rest - 1u;
        }
    };
    auto tighten = [&](Mine& m) {
        const uint64_t local_thr = compact_candidates<kBlock, Cfg::kCandPerThread>(m.s_cand, m.s_count, topk, false, s_sel);
        if (local_thr > m.thr) {
            m.thr = q8_uniform(local_thr);
            if (m.hq.ok) {
                const float local_cut = ordered_to_score(static_cast<uint32_t>(m.thr >> 32)) - m.hq.margin;
                m.cutoff = q8_uniform(local_cut > m.cutoff ? local_cut : m.cutoff);
                m.cut_d = q8_uniform(q8_threshold(m.cutoff));
                m.neg_cut = q8_uniform(q8_pair_neg_cut(m.cut_d));
            }
        }
    };

    auto process_tile = [&](const HalfTile& t, int it) {
        const int64_t quad = quad_begin + static_cast<int64_t>(it) * quad_stride;
        const int64_t r0 = quad * 4;
        // Most tiles hold no candidate of either query for a whole wave: all they pay for is the question "does any of the
        // lane's four rows reach either cut" — the largest of the eight excesses — and which rows they are is worked out
        // only where some lane answers yes.
        int ea[4], eb[4];
        q8_pair_excess4(A.hq, A.neg_cut, t, ea);
        q8_pair_excess4(B.hq, B.neg_cut, t, eb);
        const bool special[4] = {(t.t0.x & 0xffu) == kQ8Special, (t.t0.w & 0xffu) == kQ8Special, (t.t1.z & 0xffu) == kQ8Special,
                                 (t.t2.y & 0xffu) == kQ8Special};
        int top = ea[0] > eb[0] ? ea[0] : eb[0];
#pragma unroll
        for (int u = 1; u < 4; ++u) {
            top = ea[u] > top ? ea[u] : top;
            top = eb[u] > top ? eb[u] : top;
        }
        const uint64_t maybe = __ballot(top >= 0 || special[0] || special[1] || special[2] || special[3]);
        consume();   // the rows fetched while the previous tile was scanned
        if (maybe) {   // uniform
            uint32_t hit_a = 0u, hit_b = 0u;   // which of the lane's four rows each query cannot rule out
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                hit_a |= (special[u] | (ea[u] >= 0)) ? (1u << u) : 0u;
                hit_b |= (special[u] | (eb[u] >= 0)) ? (1u << u) : 0u;
            }
            const int64_t left = n - r0;
            const int valid = quad < n_quads ? (left < 4 ? static_cast<int>(left) : 4) : 0;
            const uint32_t inside = (1u << valid) - 1u;   // (padding of the last quad, the clamped prefetch past the end)
            fetch(hit_a & inside, hit_b & inside, r0);
        }
        __syncthreads();
        const int ca = *A.s_count, cb = *B.s_count;
        __syncthreads();
        if (ca >= compact_at) tighten(A);   // uniform
        if (cb >= compact_at) tighten(B);   // uniform
    };

    for (int it = 0; it < iters; it += kDepth) {
#pragma unroll
        for (int sidx = 0; sidx < kDepth; ++sidx) {
            load_tile(ring[(sidx + kDepth - 1) % kDepth], it + sidx + kDepth - 1);
            __builtin_amdgcn_sched_barrier(0);   // (the next tile is asked for before this one's first dot waits for it)
            if (it + sidx < iters) process_tile(ring[sidx], it + sidx);  // uniform
        }
    }
    consume();   // the last tile's fetches

    if (lane == 0 && A.n_rescored + B.n_rescored) atomicAdd(&sm->rescored, A.n_rescored + B.n_rescored);
    __syncthreads();
    if (tid == 0) rescored[vb] += static_cast<unsigned long long>(sm->rescored);   // launches of a handle are stream-ordered
    auto finish = [&](Mine& m, uint64_t* block_lists) {
        if (*m.s_count > kRankCountMax && *m.s_count > topk)  // uniform
            compact_candidates<kBlock, Cfg::kCandPerThread>(m.s_cand, m.s_count, topk, false, s_sel);
        __syncthreads();
        block_rank_and_store<kBlock>(m.s_cand, *m.s_count, block_lists + static_cast<int64_t>(bid) * topk, topk);
        __syncthreads();
    };
    finish(A, arg_a.block_lists);
    finish(B, arg_b.block_lists);
}

}  // namespace mi355
