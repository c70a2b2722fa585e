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
//
// GROUP CAPS (include/mi355rec_diag.h, "GROUP CAPS"): groups != null adds "at most max_per_group picks per group id >= 0".
// Thread i keeps its row's group and the number of picked rows of that group in registers; the groups also sit in LDS, so
// the winner's group is one more broadcast read next to its features; a thread whose count reaches the cap retires.  A
// step in which no wave has a live lane leaves every wave key 0 and ends the loop for all threads at once: the number of
// picks is known only at run time.  lambda == 1.0f with groups takes no loop at all (mmr_i = rel_i and the picks are the
// pool in order): rank inside the group by broadcast reads of the earlier positions' groups, keep the rows whose rank is
// below the cap, a workgroup-wide prefix sum over the kept rows (ballot, popcount, wave totals in LDS) gives the slot.
// 128 B of kernel arguments, no scratch: nothing is indexed dynamically in registers.
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
    alignas(16) int grp[kMmrBlockMax];     // the pool rows' groups (GROUP CAPS; -1 where there is no row), read as int4
    int first_empty;
};
static_assert(sizeof(MmrSmem) <= 64 * 1024, "mmr_rerank_kernel's LDS is static: 64 KB at most");

// keys[0..pool): sorted pool keys (score image << 32 | ~global row), 0-padded.  rows: this shard's matrix (n rows from global
// row `row_base`), or — staged != 0 — `pool` rows in pool order.  groups: null, or one int32 per row of `rows` (so, staged,
// the pool's groups in pool order).  out_pool_rows: null, or where P' goes.  Launch: 1 workgroup of (pool rounded up to 64) threads.
__global__ __launch_bounds__(kMmrBlockMax) void mmr_rerank_kernel(
    const uint64_t* __restrict__ keys, const float* __restrict__ rows, int64_t n, int64_t row_base, int staged, int pool, int topn,
    float lambda, float mu, int64_t* __restrict__ out_idx, float* __restrict__ out_score, float* __restrict__ out_mmr,
    float* __restrict__ rows_out, uint32_t* done_word, uint32_t done_value, const int32_t* __restrict__ groups, int max_per_group,
    int* __restrict__ out_pool_rows) {
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
    float f[kDim];
    row_features(r, f);
#pragma unroll
    for (int j = 0; j < kDim; ++j) sm.feat[j][tid] = f[j];
    sm.qn[tid] = query_norm(f);
    const bool capped = groups != nullptr;                // uniform
    const int g = capped && have ? groups[local] : -1;
    if (capped) sm.grp[tid] = g;
    __syncthreads();
    const int p_eff = sm.first_empty;                     // P'
    int picks = topn < p_eff ? topn : p_eff;              // (capped: at most so many)
    bool live = tid < p_eff;
    if (tid == 0 && out_pool_rows) *out_pool_rows = p_eff;
    const float rel = ordered_to_score(static_cast<uint32_t>(key >> 32));   // (-0.0 is +0.0 in the image already)
    const bool in_order = capped && lambda == 1.0f;       // uniform: the picks are the pool in order, no loop
    if (in_order) {
        // rank inside the group: the earlier pool positions of the same group (every position below a live one holds a row)
        int rank = 0;
        if (live && g >= 0) {
            const int4* g4 = reinterpret_cast<const int4*>(sm.grp);
            for (int j = 0; j < tid; j += 4) {   // (one address per wave: a broadcast; the trip count differs by lane)
                const int4 v = g4[j >> 2];
                rank += (v.x == g) + (j + 1 < tid && v.y == g) + (j + 2 < tid && v.z == g) + (j + 3 < tid && v.w == g);
            }
        }
        const bool keep = live && (g < 0 || rank < max_per_group);
        const uint64_t kept = __ballot(keep);
        if (lane == 0) sm.wave_key[0][wave] = static_cast<uint64_t>(__popcll(kept));
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < n_waves; ++w) {
            const int c = static_cast<int>(sm.wave_key[0][w]);
            before += w < wave ? c : 0;
            total += c;
        }
        const int slot = before + __popcll(kept & ((1ull << lane) - 1ull));
        picks = topn < total ? topn : total;
        if (keep && slot < topn) {
            out_idx[slot] = static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(key)));
            out_score[slot] = rel;
            if (out_mmr) out_mmr[slot] = rel;   // fl(fl(1 rel) - fl(0 pen)) = rel
        }
        for (int t = picks + tid; t < topn; t += static_cast<int>(blockDim.x)) {
            out_idx[t] = -1;
            out_score[t] = 0.0f;
            if (out_mmr) out_mmr[t] = 0.0f;
        }
    }
    const float a = lambda * rel;
    float pen = 0.0f;
    int seen = 0;

    for (int t = 0; !in_order && t < picks; ++t) {   // uniform trip count: every lane takes part in the DPP steps and the barrier
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
        if (best == 0ull) {   // uniform (capped only): no row is eligible any more
            picks = t;
            break;
        }
        const int p = kMmrBlockMax - 1 - static_cast<int>(static_cast<uint32_t>(best));
        if (tid == p) {
            live = false;
            sm.pick_pos[t] = static_cast<unsigned short>(p);
            sm.pick_mmr[t] = mmr;
        }
        if (capped) {   // uniform
            const int gp = sm.grp[p];
            if (gp >= 0 && g == gp && ++seen >= max_per_group) live = false;
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
    for (int t = tid; !in_order && t < topn; t += static_cast<int>(blockDim.x)) {
        const bool got = t < picks;
        const uint64_t k = got ? keys[sm.pick_pos[t]] : 0ull;
        out_idx[t] = got ? static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(k))) : -1;
        out_score[t] = got ? ordered_to_score(static_cast<uint32_t>(k >> 32)) : 0.0f;
        if (out_mmr) out_mmr[t] = got ? sm.pick_mmr[t] : 0.0f;
    }
    if (done_word) {   // uniform
        if (in_order || tid < ((topn + 63) & ~63)) __threadfence_system();   // the waves that stored results order them before ...
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done_word, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // ... the word
    }
}

}  // namespace mi355
