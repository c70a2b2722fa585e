// diverse.hip.h — DIVERSIFIED TOP-N (include/mi355rec_diag.h): maximal marginal relevance over a relevance pool.
//
// mmr_rerank_kernel: ONE workgroup picks `topn` of the P' <= 1024 pool rows greedily.  Thread i owns pool position i: its
// row's 12 features, its relevance and its penalty stay in registers for the whole loop; LDS holds the rows TRANSPOSED
// (feature-major, s_feat[j][i]: the gather's stores and the loop's reads are conflict-free — lanes write consecutive
// words, and a picked row is read by every lane at one address, a broadcast), the picked rows' norms and the picks.
// Per pick: every lane forms mmr = fl(fl(lambda rel) - fl(mu pen)), the wave takes its arg-max in DPP (wave_max_u32 on the
// order-preserving image, then the lowest lane that holds it: the earlier pool position wins a tie), lane 0 of every wave
// leaves (image << 32 | 1023 - position) in LDS, ONE barrier (the wave slots are double-buffered by the pick's parity), every
// lane reads the <= 16 wave keys and knows the winner; it then runs the exact chain of the scans (cosine_score, core.hip.h)
// for its row against the picked row and raises its penalty.  N - 1 dependent steps: the loop is latency, not throughput.
// After the loop thread t writes pick t (id, relevance, mmr) to the caller's buffers — the handle's pinned result slots —
// and the completion word follows as in the notifying form of merge_kernel (merge.hip.h).
//
// The same kernel serves two more callers by flags instead of instantiations (the library keeps to sixty kernels):
//   staged   rows[i] is pool row i, passed by value (a row-sharded node gathers the pool from its shards first);
//   rows_out the gather alone: row i of the listed keys is stored to rows_out[i] and nothing is ranked
//            (mi355rec_fetch_rows).
// 104 B of kernel arguments, no scratch: nothing is indexed dynamically in registers.
#pragma once

#include "core.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kMmrBlockMax = kMaxTopK;   // one thread per pool row
constexpr int kMmrWavesMax = kMmrBlockMax / 64;

struct MmrSmem {
    float feat[kDim][kMmrBlockMax];        // 48 KB, feature-major
    float qn[kMmrBlockMax];                // |row i| as a query (query_norm)
    float pick_mmr[kMmrBlockMax];
    unsigned short pick_pos[kMmrBlockMax];
    uint64_t wave_key[2][kMmrWavesMax];
    int first_empty;
};

// keys[0..pool): sorted pool keys (score image << 32 | ~global row), 0-padded.  rows: this shard's matrix (n rows from global
// row `row_base`), or — staged != 0 — `pool` rows in pool order.  Launch: 1 workgroup of (pool rounded up to 64) threads.
__global__ __launch_bounds__(kMmrBlockMax) void mmr_rerank_kernel(
    const uint64_t* __restrict__ keys, const float* __restrict__ rows, int64_t n, int64_t row_base, int staged, int pool, int topn,
    float lambda, float mu, int64_t* __restrict__ out_idx, float* __restrict__ out_score, float* __restrict__ out_mmr,
    float* __restrict__ rows_out, uint32_t* done_word, uint32_t done_value) {
    __shared__ MmrSmem sm;
    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n_waves = static_cast<int>(blockDim.x + 63) >> 6;

    const uint64_t key = tid < pool ? keys[tid] : 0ull;
    const int64_t local = staged ? static_cast<int64_t>(tid)
                                 : static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(key))) - row_base;
    // (a key that names no row of `rows` is treated as the end of the pool: nothing is read out of bounds)
    const bool have = key != 0ull && local >= 0 && (staged ? tid < pool : local < n);
    Row r;
    r.a = r.b = r.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (have) r = load_row(rows, local);

    if (rows_out) {   // uniform: the gather alone
        if (have) {
            float4* o = reinterpret_cast<float4*>(rows_out + static_cast<int64_t>(tid) * kDim);
            o[0] = r.a;
            o[1] = r.b;
            o[2] = r.c;
        }
        return;
    }

    if (tid == 0) sm.first_empty = pool < static_cast<int>(blockDim.x) ? pool : static_cast<int>(blockDim.x);
    __syncthreads();
    if (!have && tid < pool) atomicMin(&sm.first_empty, tid);
    const float f[kDim] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x, r.c.y, r.c.z, r.c.w};
#pragma unroll
    for (int j = 0; j < kDim; ++j) sm.feat[j][tid] = f[j];
    sm.qn[tid] = query_norm(f);
    __syncthreads();
    const int p_eff = sm.first_empty;                     // P'
    const int picks = topn < p_eff ? topn : p_eff;
    bool live = tid < p_eff;
    const float rel = ordered_to_score(static_cast<uint32_t>(key >> 32));   // (-0.0 is +0.0 in the image already)
    const float a = lambda * rel;
    float pen = 0.0f;

    for (int t = 0; t < picks; ++t) {   // uniform trip count: every lane takes part in the DPP steps and the barrier
        const float b = mu * pen;
        const float mmr = a - b;
        const uint32_t img = live ? score_to_ordered(mmr) : 0u;   // (an image of a finite score is never 0)
        const uint32_t best_img = wave_max_u32(img);
        const uint64_t who = __ballot(live && img == best_img);
        if (lane == 0) {
            const int pos = wave * 64 + (__ffsll(static_cast<long long>(who)) - 1);
            sm.wave_key[t & 1][wave] = who ? (static_cast<uint64_t>(best_img) << 32) | static_cast<uint32_t>(kMmrBlockMax - 1 - pos) : 0ull;
        }
        __syncthreads();
        uint64_t best = 0ull;
        for (int w = 0; w < n_waves; ++w) {
            const uint64_t k = sm.wave_key[t & 1][w];
            best = k > best ? k : best;
        }
        const int p = kMmrBlockMax - 1 - static_cast<int>(static_cast<uint32_t>(best));
        if (tid == p) {
            live = false;
            sm.pick_pos[t] = static_cast<unsigned short>(p);
            sm.pick_mmr[t] = mmr;
        }
        if (t + 1 < picks) {   // uniform
            float q[kDim];
#pragma unroll
            for (int j = 0; j < kDim; ++j) q[j] = sm.feat[j][p];
            const float c = cosine_score(q, sm.qn[p], r);   // row i scanned, row p the query
            pen = c > pen ? c : pen;
        }
    }
    __syncthreads();
    for (int t = tid; t < topn; t += static_cast<int>(blockDim.x)) {
        const bool got = t < picks;
        const uint64_t k = got ? keys[sm.pick_pos[t]] : 0ull;
        out_idx[t] = got ? static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(k))) : -1;
        out_score[t] = got ? ordered_to_score(static_cast<uint32_t>(k >> 32)) : 0.0f;
        if (out_mmr) out_mmr[t] = got ? sm.pick_mmr[t] : 0.0f;
    }
    if (done_word) {   // uniform
        if (tid < ((topn + 63) & ~63)) __threadfence_system();   // the waves that stored results order them before ...
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done_word, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // ... the word
    }
}

}  // namespace mi355
