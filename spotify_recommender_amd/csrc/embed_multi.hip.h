// embed_multi.hip.h — the kernels of libmi355rec_embed_multi.so (gfx950 only; include/mi355rec_embed_multi.h): ONE pass
// over an embedding table for the K <= 32 interests of one user, one candidate list, one key per row.
//
// embed_multi_scan_kernel<Rows, kDimT> keeps embed_scan_body's streaming (embed.hip.h): 512 threads, thread t loads the Vec
// at vector index tile * kEmbedTileVecs + j * kEmbedBlock + t, G = kDimT / Rows::kVals consecutive lanes hold one row, two
// tiles of four loads are in flight per lane, the xor-butterflies of embed_tree_levels leave a tree sum in every lane of the
// group.  It keeps that body's selection too: one candidate list per workgroup, the exclusion list in LDS, the two-barrier
// count read, compaction at compact_at, block_rank_and_store into block_lists[grid][topk]; merge_kernel follows.
//   What the interests share: the load, the widening, the row's nn = tree(e, e) and sqrtf(nn) (once per loaded row), and
// everything behind the value — one key, one threshold test, one exclusion search, one append.  What each interest adds: one
// dot tree, and 1 / min(G, K) of a tail (division, clamp, blend).  The tail is DEALT over the lanes of a group, as
// embed_batch_scan_kernel deals its users': after the butterflies every lane of a group holds every dot, so the interests
// are taken in ROUNDS of G, lane g keeps the dot of interest r0 + g (one select per dot), finishes that one interest per
// load, and a max-butterfly over the group (embed_multi_group_max: the tree's exchanges with max for +) leaves the round's
// largest finite value in every lane.
//   The interests are staged once per workgroup in LDS (<= 16 KiB at K = 32, d = 128) in the layout each lane reads them
// back in — float4 plane `part` of interest k at s_int[(k * kParts + part) * G + g], kParts = Rows::kVals / 4, so the lanes
// of a group read consecutive 16-byte words and equal g broadcast — with nu_k = sqrtf(tree(u_k, u_k)) beside them.  Within a
// round they are consumed in CHUNKS of kEmbedMultiPass: a chunk's vectors go from LDS into registers once per tile and serve
// its four loads; each load's lane carries the running maximum `best[j]` from round to round.  A lane past the last
// interest — a padded slot of a short last chunk (staged as zeros, which would score c = 0 and beat every negative value) or
// a round the request does not fill — never takes part in the maximum: it enters the butterfly with -inf.
//   V and the interest: best starts at -inf; a lane's value enters the butterfly if it is finite, else as -inf; best ends as
// the largest finite v_k, and best == -inf says no v_k was finite and the row forms no key.  -0.0 and +0.0 compare equal, so
// either may come out of a butterfly: pack_key reports both as +0.0.
// The scan needs V alone.  The key has no room for k, so embed_multi_finish_kernel recomputes it for the winners.
//
// embed_multi_finish_kernel does what embed_stream_finish_kernel does (ids, scores, count, padding) and, with out_interest,
// stages the interests and their norms in LDS once, re-reads each of the `count` winning rows (and its audio_s word), forms
// the K values with the same functions as the scan — G lanes per winner, 256 / G winners per step — and stores the lowest
// argmax: at most 1024 x 32 trees, off the bandwidth path.  One kernel serves every layout: a uniform switch picks the instantiation of its body.
#pragma once

#include "embed_stream.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kEmbedMultiMaxInterests = 32;   // MI355REC_EMBED_MULTI_MAX_INTERESTS
#ifndef MI355REC_EMBED_MULTI_PASS
#define MI355REC_EMBED_MULTI_PASS 2
#endif
constexpr int kEmbedMultiPass = MI355REC_EMBED_MULTI_PASS;   // interests in registers at a time
constexpr int kEmbedMultiFinishBlock = 256;
static_assert(kEmbedMultiPass >= 1 && (kEmbedMultiPass & (kEmbedMultiPass - 1)) == 0 && kEmbedMultiMaxInterests % kEmbedMultiPass == 0,
              "a power of two that divides 32");

struct EmbedMultiArgs {
    EmbedArgs a;
    int n_interests;   // 1 .. kEmbedMultiMaxInterests
};

// v_k of one row from its dot with interest k: the contract's tail.  sq = sqrtf(nn) of the row (cosine only), nu = the
// interest's norm, s = the row's audio cosine (use_audio only).
__device__ __forceinline__ float embed_multi_value(float dot, float sq, float nu, float s, const EmbedArgs& a) {
    float c = dot;
    if (a.metric == 0) {   // uniform
        const float den = sq * nu;
        c = 0.0f;
        if (den > 1e-8f) {
            const float t = dot / den;
            const float m = (t < 1.0f) ? t : 1.0f;
            c = (-1.0f < m) ? m : -1.0f;
        }
    }
    float v = a.w_embed * c;
    if (a.use_audio) {
        const float wa = a.w_audio * s;
        v = wa + v;
    }
    return v;
}

// The largest x over the kGroup lanes of a row, in every lane of the group (embed_tree_levels' exchanges with max for +;
// no x is a NaN).
template <int kGroup>
__device__ __forceinline__ float embed_multi_group_max(float x) {
    auto larger = [](float p, float q) { return p > q ? p : q; };
    x = larger(x, embed_dpp_xor1(x));
    if constexpr (kGroup >= 4) x = larger(x, embed_dpp_xor2(x));
    if constexpr (kGroup >= 8) x = larger(x, embed_dpp_half_mirror(x));
    if constexpr (kGroup >= 16) x = larger(x, embed_dpp_mirror(x));
    if constexpr (kGroup >= 32) x = larger(x, __shfl_xor(x, 16, 64));
    return x;
}

// Interest k's values of lane g from the staged planes.
template <class Rows>
__device__ __forceinline__ typename Rows::Row embed_multi_staged(const float4* s_int, int k, int g, int group) {
    if constexpr (Rows::kVals == 4) {
        return s_int[k * group + g];
    } else {
        return {s_int[(2 * k) * group + g], s_int[(2 * k + 1) * group + g]};
    }
}

// table: n x kDimT Rows::Word (n >= 1); interests: m.n_interests x kDimT floats; audio_s: n floats or null (use_audio == 0);
// exclude: n_exclude sorted local rows; block_lists[gridDim.x][topk].
template <class Rows, int kDimT>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_multi_scan_kernel(
    const typename Rows::Word* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ interests, const float* __restrict__ audio_s,
    const uint32_t* __restrict__ exclude, EmbedMultiArgs m, uint64_t* __restrict__ block_lists) {
    using Vec = typename Rows::Vec;
    using Row = typename Rows::Row;
    constexpr int kGroup = kDimT / Rows::kVals;                        // lanes per row
    constexpr int kParts = Rows::kVals / 4;                            // float4 planes of a lane's values
    constexpr int kTileRows = kEmbedTileVecs / kGroup;
    constexpr int kMaxTileRows = kEmbedTileVecs / (16 / Rows::kVals);   // d = 16
    constexpr int kCandCap = kCandLimit + kMaxTileRows;
    constexpr int kCandPerThread = (kCandCap + kEmbedBlock - 1) / kEmbedBlock;
    constexpr int kIntVecs = kEmbedMultiMaxInterests * kDimT / 4;      // float4 words of 32 staged interests
    constexpr int kGroupsPerBlock = kEmbedBlock / kGroup;
    constexpr int kP = kEmbedMultiPass < kGroup ? kEmbedMultiPass : kGroup;   // (a chunk lies inside a round)
    static_assert(kGroup >= 2 && kGroup <= 32 && 64 % kGroup == 0, "a row lies inside one wave");
    static_assert(kTileRows <= kMaxTileRows, "a tile appends at most kMaxTileRows candidates");
    static_assert(kCandPerThread * kEmbedBlock >= kCandCap, "compact_candidates reads the whole list");
    static_assert(2 * kGroupsPerBlock >= kEmbedMultiMaxInterests, "two rounds of the workgroup's groups norm every interest");
    __shared__ uint64_t s_cand[kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count;
    __shared__ uint32_t s_excl[kEmbedMaxExclude];
    __shared__ float4 s_int[kIntVecs];
    __shared__ float s_nu[kEmbedMultiMaxInterests];

    const EmbedArgs a = m.a;
    const int K = m.n_interests;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = tid & (kGroup - 1);
    const int64_t n_vec = n * kGroup;
    const Vec* const tab4 = reinterpret_cast<const Vec*>(table);
    const int64_t n_tiles = (n_vec + kEmbedTileVecs - 1) / kEmbedTileVecs;

    auto load_tile = [&](int64_t tile, Vec (&e)[kEmbedVecsPerThread], float (&s)[kEmbedVecsPerThread]) {
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            int64_t v = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            v = v < n_vec ? v : n_vec - 1;   // (a clamped lane's row is never used: rows are whole groups of lanes)
            e[j] = tab4[v];
            s[j] = a.use_audio ? audio_s[v / kGroup] : 0.0f;
        }
    };
    auto tree = [](const Row& x, const Row& y) { return embed_tree_levels<kGroup>(Rows::partial(x, y)); };

    int64_t tile = blockIdx.x;
    Vec cur_e[kEmbedVecsPerThread];
    float cur_s[kEmbedVecsPerThread];
    if (tile < n_tiles) load_tile(tile, cur_e, cur_s);   // requested before the interests are

    if (tid == 0) s_count = 0;
    for (int i = tid; i < a.n_exclude; i += kEmbedBlock) s_excl[i] = exclude[i];
    // the interests into their planes; the slots of a short last chunk are zeros
    const int k_staged = (K + kP - 1) / kP * kP;
    for (int i = tid; i < k_staged * (kDimT / 4); i += kEmbedBlock) {
        const int k = i / (kDimT / 4);
        const int q = i - k * (kDimT / 4);   // float4 q of interest k: plane q % kParts of lane q / kParts
        const float4 w = k < K ? reinterpret_cast<const float4*>(interests)[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_int[(k * kParts + q % kParts) * kGroup + q / kParts] = w;
    }
    __syncthreads();
#pragma unroll
    for (int round = 0; round < 2; ++round) {   // every lane takes part in the butterflies; a group past the last interest stores nothing
        const int k = round * kGroupsPerBlock + tid / kGroup;
        const Row u = embed_multi_staged<Rows>(s_int, k < k_staged ? k : 0, g, kGroup);
        const float nu = sqrtf(tree(u, u));
        if (g == 0 && k < k_staged) s_nu[k] = nu;
    }
    __syncthreads();

    uint64_t thr = 0;
    int compact_at = 2 * a.topk > 256 ? 2 * a.topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;

    for (; tile < n_tiles; tile += gridDim.x) {   // uniform
        const int64_t next_tile = tile + gridDim.x;
        Vec next_e[kEmbedVecsPerThread];
        float next_s[kEmbedVecsPerThread];
        load_tile(next_tile < n_tiles ? next_tile : tile, next_e, next_s);   // the next tile is in flight while this one is scored

        float sq[kEmbedVecsPerThread], best[kEmbedVecsPerThread];
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            best[j] = -INFINITY;
            sq[j] = 0.0f;
            if (a.metric == 0) {   // uniform; once per loaded row
                const Row e = Rows::widen(cur_e[j]);
                sq[j] = sqrtf(tree(e, e));
            }
        }
#pragma unroll 1
        for (int r0 = 0; r0 < K; r0 += kGroup) {   // uniform: the rounds of kGroup interests, lane g finishes interest r0 + g
            float mine[kEmbedVecsPerThread];
#pragma unroll
            for (int j = 0; j < kEmbedVecsPerThread; ++j) mine[j] = 0.0f;
#pragma unroll 1
            for (int c = 0; c < kGroup && r0 + c < K; c += kP) {   // uniform: the chunks of the round
                Row u[kP];
                bool own[kP];
#pragma unroll
                for (int p = 0; p < kP; ++p) {
                    u[p] = embed_multi_staged<Rows>(s_int, r0 + c + p, g, kGroup);
                    own[p] = g == c + p;
                }
#pragma unroll
                for (int j = 0; j < kEmbedVecsPerThread; ++j) {
                    const Row e = Rows::widen(cur_e[j]);
#pragma unroll
                    for (int p = 0; p < kP; ++p) {
                        const float dot = tree(e, u[p]);   // in every lane of the group: the one that finishes it keeps it
                        mine[j] = own[p] ? dot : mine[j];
                    }
                }
            }
            // a lane past the last interest (a padded slot of a short chunk, or a round the request does not fill) holds -inf
            const int kk = r0 + g;
            const bool real = kk < K;
            const float nu = s_nu[real ? kk : 0];
#pragma unroll
            for (int j = 0; j < kEmbedVecsPerThread; ++j) {
                const float v = embed_multi_value(mine[j], sq[j], nu, cur_s[j], a);
                const float round_max = embed_multi_group_max<kGroup>(real && __builtin_isfinite(v) ? v : -INFINITY);
                if (round_max > best[j]) best[j] = round_max;
            }
        }

#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            const int64_t vec = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            const int64_t row = vec / kGroup;
            const bool owner = g == 0 && vec < n_vec;
            uint64_t key = 0;
            if (owner && best[j] > -INFINITY) key = pack_key(best[j], static_cast<uint32_t>(row_base + row));
            bool pass = key > thr;
            if (pass && a.n_exclude > 0) {   // (rare once the threshold stands: a binary search over the sorted list in LDS)
                const uint32_t local = static_cast<uint32_t>(row);
                int lo = 0, hi = a.n_exclude;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_excl[mid] < local) lo = mid + 1;
                    else hi = mid;
                }
                pass = !(lo < a.n_exclude && s_excl[lo] == local);
            }
            const uint64_t ballot = __ballot(pass);
            if (ballot) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&s_count, __popcll(ballot));
                base = __builtin_amdgcn_readfirstlane(base);
                if (pass) s_cand[base + lanes_below(ballot)] = key;
            }
        }
        // two barriers: every wave reads the count before any wave appends again (scan_kernel)
        __syncthreads();
        const int c = s_count;
        __syncthreads();
        if (c >= compact_at) {
            const uint64_t local_thr = compact_candidates<kEmbedBlock, kCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
            if (local_thr > thr) thr = local_thr;
        }
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            cur_e[j] = next_e[j];
            cur_s[j] = next_s[j];
        }
    }

    __syncthreads();
    if (s_count > kRankCountMax && s_count > a.topk)   // uniform
        compact_candidates<kEmbedBlock, kCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kEmbedBlock>(s_cand, s_count, block_lists + static_cast<int64_t>(blockIdx.x) * a.topk, a.topk);
}

// What the finish kernel is given beside the keys and the outputs: the table and the request, to recompute the interests.
struct EmbedMultiFinishArgs {
    const void* table;
    int64_t n;
    int64_t row_base;
    const float* interests;
    const float* audio_s;
    EmbedMultiArgs m;
    int storage;   // MI355REC_EMBED_STREAM_FP32 (-1), MI355REC_EMBED_HALF_FP16 / _BF16
    int dim;
};

// The interest of each of the `count` winners of keys[] into out_interest: kGroup lanes per winner.  s_u (the workgroup's
// 32 x 128 floats) and s_nu take the interests and their norms once, as the scan stages them: a winner's K values then read LDS.
template <class Rows, int kDimT>
__device__ __forceinline__ void embed_multi_attribute(const uint64_t* __restrict__ keys, int count, const EmbedMultiFinishArgs& f,
                                                      int32_t* __restrict__ out_interest, float4* s_u, float* s_nu) {
    using Vec = typename Rows::Vec;
    using Row = typename Rows::Row;
    constexpr int kGroup = kDimT / Rows::kVals;
    constexpr int kPerStep = kEmbedMultiFinishBlock / kGroup;
    const EmbedArgs a = f.m.a;
    const int t = threadIdx.x;
    const int g = t & (kGroup - 1);
    auto tree = [](const Row& x, const Row& y) { return embed_tree_levels<kGroup>(Rows::partial(x, y)); };
    const int K = f.m.n_interests;
    const float* const s_interests = reinterpret_cast<const float*>(s_u);   // row-major, as given
    for (int i = t; i < K * (kDimT / 4); i += kEmbedMultiFinishBlock) s_u[i] = reinterpret_cast<const float4*>(f.interests)[i];
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += kPerStep) {   // uniform: a group past the last interest norms interest 0 again and stores nothing
        const int k = k0 + t / kGroup;
        const Row u = Rows::user(s_interests + (k < K ? k : 0) * kDimT, g);
        const float nu = sqrtf(tree(u, u));
        if (g == 0 && k < K) s_nu[k] = nu;
    }
    __syncthreads();
    for (int base = 0; base < count; base += kPerStep) {   // uniform: every lane takes part in the butterflies
        const int i = base + t / kGroup;
        const bool valid = i < count;
        // the key holds ~(uint32_t)(row_base + row): the local row comes back modulo 2^32 (a lane past the last winner reads row 0)
        const uint32_t global = valid ? ~static_cast<uint32_t>(keys[i]) : static_cast<uint32_t>(f.row_base);
        int64_t row = static_cast<int64_t>(static_cast<uint32_t>(global - static_cast<uint32_t>(f.row_base)));
        row = row < f.n ? row : 0;   // (never taken for a key the scan formed)
        const Row e = Rows::widen(reinterpret_cast<const Vec*>(f.table)[row * kGroup + g]);
        const float s = a.use_audio ? f.audio_s[row] : 0.0f;
        const float sq = a.metric == 0 ? sqrtf(tree(e, e)) : 0.0f;
        float best = -INFINITY;
        int best_k = -1;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {   // uniform
            const Row u = Rows::user(s_interests + k * kDimT, g);
            const float v = embed_multi_value(tree(e, u), sq, s_nu[k], s, a);
            if (__builtin_isfinite(v) && v > best) {   // (strict: the lowest k holds an equal value)
                best = v;
                best_k = k;
            }
        }
        if (valid && g == 0) out_interest[i] = best_k;
    }
}

template <class Rows>
__device__ __forceinline__ void embed_multi_attribute_rows(const uint64_t* __restrict__ keys, int count, const EmbedMultiFinishArgs& f,
                                                           int32_t* __restrict__ out_interest, float4* s_u, float* s_nu) {
    switch (f.dim) {   // uniform
        case 16: embed_multi_attribute<Rows, 16>(keys, count, f, out_interest, s_u, s_nu); break;
        case 32: embed_multi_attribute<Rows, 32>(keys, count, f, out_interest, s_u, s_nu); break;
        case 64: embed_multi_attribute<Rows, 64>(keys, count, f, out_interest, s_u, s_nu); break;
        default: embed_multi_attribute<Rows, 128>(keys, count, f, out_interest, s_u, s_nu); break;
    }
}

// keys: eff merged keys (eff >= 0; sorted descending, 0 behind the last); out_idx / out_score / out_interest: topn; out_score,
// out_count and out_interest may be null.  One workgroup.
__global__ __launch_bounds__(kEmbedMultiFinishBlock) void embed_multi_finish_kernel(
    const uint64_t* __restrict__ keys, int eff, int topn, int64_t* __restrict__ out_idx, float* __restrict__ out_score, int32_t* __restrict__ out_count,
    int32_t* __restrict__ out_interest, EmbedMultiFinishArgs f) {
    __shared__ int s_count;
    __shared__ float4 s_u[kEmbedMultiMaxInterests * MI355REC_EMBED_MAX_DIM / 4];
    __shared__ float s_nu[kEmbedMultiMaxInterests];
    const int t = threadIdx.x;
    if (t == 0) s_count = 0;
    __syncthreads();
    for (int base = 0; base < eff; base += kEmbedMultiFinishBlock) {   // uniform
        const int i = base + t;
        const uint64_t there = __ballot(i < eff && keys[i] != 0ull);
        if ((t & 63) == 0 && there) atomicAdd(&s_count, __popcll(there));
    }
    __syncthreads();
    const int count = s_count;
    for (int i = t; i < topn; i += kEmbedMultiFinishBlock) {
        const bool have = i < count;
        const uint64_t key = have ? keys[i] : 0ull;
        out_idx[i] = have ? static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(key))) : static_cast<int64_t>(-1);
        if (out_score) out_score[i] = have ? ordered_to_score(static_cast<uint32_t>(key >> 32)) : 0.0f;
        if (out_interest && !have) out_interest[i] = -1;
    }
    if (out_count && t == 0) out_count[0] = count;
    if (!out_interest || count == 0) return;   // uniform
    if (f.storage == MI355REC_EMBED_HALF_FP16) embed_multi_attribute_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_FP16>>(keys, count, f, out_interest, s_u, s_nu);
    else if (f.storage == MI355REC_EMBED_HALF_BF16) embed_multi_attribute_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_BF16>>(keys, count, f, out_interest, s_u, s_nu);
    else embed_multi_attribute_rows<EmbedRowsF32>(keys, count, f, out_interest, s_u, s_nu);
}

}  // namespace mi355
