// embed_batch.hip.h — the kernel of libmi355rec_embed_batch.so (gfx950 only): ONE pass over an embedding table for up to
// kPassT users (include/mi355rec_embed_batch.h; the arithmetic is include/mi355rec_embed.h's, bit for bit).
//
// embed_batch_scan_kernel<kDimT, kPassT> has embed_scan_kernel's shape (embed.hip.h): 512 threads, thread t loads the float4
// at vector index tile * kEmbedTileVecs + j * kEmbedBlock + t, G = kDimT / 4 consecutive lanes hold one row, two tiles of
// four loads are in flight per lane, the xor-butterflies of embed_tree_levels leave a tree sum in every lane of the group.
// What the users of a pass share: the load, the row's nn = tree(e, e) and sqrtf(nn) (once per row), and the tail's
// instructions — after the butterflies every lane of a group holds every user's dot, so lane g FINISHES user g (division,
// clamp, blend, key, threshold, exclusion search, append): with G >= kPassT lanes g >= kPassT idle in the tail, with
// G < kPassT (d = 16, G = 4, eight users) a lane finishes kPassT / G users, one after the other.
// What each user adds: four multiplies, three adds and the butterfly per 16-byte load, and its four user values in registers.
//
// Per user the workgroup keeps one candidate list and one count in LDS; the user's threshold lives in the registers of the
// lanes that finish it (compact_candidates returns it to every thread).  THE INVARIANT: a tile is entered with at most
// kEmbedBatchCandLimit = 2 * 128 candidates per user, a tile appends at most kTileRows per user (one lane per row and
// user), and a list has kEmbedBatchCandLimit + kTileRows slots — so no append leaves its list.  Counts are read between
// two barriers after every tile (scan_kernel's rule: every wave reads them before any wave appends again), and a user
// whose count passed the limit is compacted (core.hip.h's compact_candidates) to at most topk + max(16, topk / 4) <= 160.
// Exclusion lists stay in device memory (sorted local rows, CSR): only a key that already passes its user's threshold
// searches them.  A short last pass runs with a.users < kPassT: the padded users' vectors are zeros and no lane forms
// their keys.
#pragma once

#include "embed.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kEmbedBatchMaxPass = 8;
constexpr int kEmbedBatchMaxTopK = 128;                          // MI355REC_EMBED_BATCH_MAX_TOPN
constexpr int kEmbedBatchCandLimit = 2 * kEmbedBatchMaxTopK;    // a tile is never entered with more candidates per user

struct EmbedBatchArgs {
    float w_embed;
    int metric;   // 0 cosine, 1 dot
    int topk;     // <= kEmbedBatchMaxTopK
    int users;    // users of this pass: 1 .. kPassT
};

// table: n x kDimT floats (n >= 1); users: kPassT x kDimT floats (rows >= a.users are zeros); excl / excl_off: the users'
// sorted local rows and a.users + 1 offsets into them, or excl_off null (nothing excluded); block_lists[a.users][gridDim.x][topk].
template <int kDimT, int kPassT>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_batch_scan_kernel(
    const float* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ users, const uint32_t* __restrict__ excl,
    const int64_t* __restrict__ excl_off, EmbedBatchArgs a, uint64_t* __restrict__ block_lists) {
    constexpr int kGroup = kDimT / 4;                                   // lanes per row
    constexpr int kTileRows = kEmbedTileVecs / kGroup;
    constexpr int kCap = kEmbedBatchCandLimit + kTileRows;              // slots of one user's list
    constexpr int kCandPerThread = (kCap + kEmbedBlock - 1) / kEmbedBlock;
    constexpr int kPerLane = kPassT > kGroup ? kPassT / kGroup : 1;      // users a lane finishes
    constexpr int kDealt = kPassT < kGroup ? kPassT : kGroup;            // lanes of a group that finish somebody
    static_assert(kGroup >= 4 && kGroup <= 32 && 64 % kGroup == 0, "a row lies inside one wave");
    static_assert(kPassT >= 1 && kPassT <= kEmbedBatchMaxPass && (kPassT & (kPassT - 1)) == 0, "1, 2, 4 or 8 users per pass");
    static_assert(kPerLane * kDealt == kPassT, "every user has exactly one lane per row");
    static_assert(kPassT * kCap * 8 + sizeof(SelectSmem) + 64 <= 65536, "64 KiB of LDS per workgroup");
    __shared__ uint64_t s_cand[kPassT * kCap];
    __shared__ SelectSmem s_sel;
    __shared__ __attribute__((aligned(16))) int s_count[kEmbedBatchMaxPass];

    const int tid = threadIdx.x;
    const int g = tid & (kGroup - 1);
    const int64_t n_vec = n * kGroup;
    const float4* const tab4 = reinterpret_cast<const float4*>(table);
    const int64_t n_tiles = (n_vec + kEmbedTileVecs - 1) / kEmbedTileVecs;

    auto load_tile = [&](int64_t tile, float4 (&e)[kEmbedVecsPerThread]) {
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            int64_t v = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            v = v < n_vec ? v : n_vec - 1;   // (a clamped lane's row is never used: rows are whole groups of lanes)
            e[j] = tab4[v];
        }
    };

    int64_t tile = blockIdx.x;
    float4 cur_e[kEmbedVecsPerThread];
    if (tile < n_tiles) load_tile(tile, cur_e);   // requested before the user vectors are

    if (tid < kEmbedBatchMaxPass) s_count[tid] = 0;
    float4 u4[kPassT];
    float nu_all[kPassT];
#pragma unroll
    for (int p = 0; p < kPassT; ++p) {
        u4[p] = reinterpret_cast<const float4*>(users)[p * kGroup + g];
        nu_all[p] = sqrtf(embed_tree_levels<kGroup>(embed_partial(u4[p], u4[p])));
    }
    // what this lane finishes: user mu[i] = g + i * kGroup of the pass (a lane with g >= kDealt, or a padded user: nobody)
    bool mine[kPerLane];
    float nu[kPerLane];
    uint64_t thr[kPerLane];
    int64_t ex_lo[kPerLane];
    int ex_n[kPerLane];
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        const int mu = g + i * kGroup;
        mine[i] = g < kDealt && mu < a.users;
        nu[i] = nu_all[i * kDealt];
#pragma unroll
        for (int q = 1; q < kDealt; ++q)
            if (g == q) nu[i] = nu_all[i * kDealt + q];
        thr[i] = 0;
        ex_lo[i] = 0;
        ex_n[i] = 0;
        if (mine[i] && excl_off) {
            ex_lo[i] = excl_off[mu];
            ex_n[i] = static_cast<int>(excl_off[mu + 1] - ex_lo[i]);
        }
    }
    __syncthreads();

    for (; tile < n_tiles; tile += gridDim.x) {   // uniform
        const int64_t next_tile = tile + gridDim.x;
        float4 next_e[kEmbedVecsPerThread];
        load_tile(next_tile < n_tiles ? next_tile : tile, next_e);   // the next tile is in flight while this one is scored

#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            const int64_t vec = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            const int64_t row = vec / kGroup;
            float dot[kPassT];
#pragma unroll
            for (int p = 0; p < kPassT; ++p) dot[p] = embed_tree_levels<kGroup>(embed_partial(cur_e[j], u4[p]));
            float sq = 0.0f;
            if (a.metric == 0) sq = sqrtf(embed_tree_levels<kGroup>(embed_partial(cur_e[j], cur_e[j])));   // uniform; once per row
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) {
                float d = dot[i * kDealt];
#pragma unroll
                for (int q = 1; q < kDealt; ++q)
                    if (g == q) d = dot[i * kDealt + q];
                float c = d;
                if (a.metric == 0) {   // uniform
                    const float den = sq * nu[i];
                    c = 0.0f;
                    if (den > 1e-8f) {
                        const float t = d / den;
                        const float m = (t < 1.0f) ? t : 1.0f;
                        c = (-1.0f < m) ? m : -1.0f;
                    }
                }
                const float v = a.w_embed * c;
                uint64_t key = 0;
                if (mine[i] && vec < n_vec && __builtin_isfinite(v)) key = pack_key(v, static_cast<uint32_t>(row_base + row));
                bool pass = key > thr[i];
                if (__ballot(pass)) {   // wave-uniform, and rare once the thresholds stand
                    const int mu = g + i * kGroup;
                    if (pass && ex_n[i] > 0) {   // a binary search over the user's sorted list in device memory
                        const uint32_t local = static_cast<uint32_t>(row);
                        const uint32_t* const list = excl + ex_lo[i];
                        int lo = 0, hi = ex_n[i];
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (list[mid] < local) lo = mid + 1;
                            else hi = mid;
                        }
                        pass = !(lo < ex_n[i] && list[lo] == local);
                    }
                    if (pass) {
                        const int slot = atomicAdd(&s_count[mu], 1);   // < kCap: THE INVARIANT above
                        s_cand[mu * kCap + slot] = key;
                    }
                }
            }
        }
        // two barriers: every wave reads the counts before any wave appends again (scan_kernel)
        __syncthreads();
        int counts[kEmbedBatchMaxPass];
        {
            const int4 lo4 = *reinterpret_cast<const int4*>(&s_count[0]);
            const int4 hi4 = *reinterpret_cast<const int4*>(&s_count[4]);
            counts[0] = lo4.x, counts[1] = lo4.y, counts[2] = lo4.z, counts[3] = lo4.w;
            counts[4] = hi4.x, counts[5] = hi4.y, counts[6] = hi4.z, counts[7] = hi4.w;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < kPassT; ++p) {
            if (counts[p] > kEmbedBatchCandLimit) {   // uniform (never a padded user: its count stays 0)
                const uint64_t t = compact_candidates<kEmbedBlock, kCandPerThread>(s_cand + p * kCap, &s_count[p], a.topk, false, s_sel);
#pragma unroll
                for (int i = 0; i < kPerLane; ++i)
                    if (g + i * kGroup == p && t > thr[i]) thr[i] = t;
            }
        }
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) cur_e[j] = next_e[j];
    }

    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < a.users; ++p) {   // uniform
        uint64_t* const list = s_cand + p * kCap;
        if (s_count[p] > kRankCountMax && s_count[p] > a.topk)   // uniform
            compact_candidates<kEmbedBlock, kCandPerThread>(list, &s_count[p], a.topk, false, s_sel);
        __syncthreads();
        block_rank_and_store<kEmbedBlock>(list, s_count[p], block_lists + (static_cast<int64_t>(p) * gridDim.x + blockIdx.x) * a.topk, a.topk);
    }
}

}  // namespace mi355
