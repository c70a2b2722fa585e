// embed_half.hip.h — the kernels of libmi355rec_embed_half.so (gfx950 only): the HYBRID scan over a HALF-PRECISION
// embedding table (include/mi355rec_embed_half.h: fp16 or bf16 words, answers those of mi355rec_embed.h's arithmetic
// contract over the widened values W(x), bit for bit) and the kernel that forms a user vector from member rows.
// embed.hip.h is included unedited: its helpers, embed_probe_kernel (raw 16-byte vectors: it reads a half table as it
// reads an fp32 one) and merge_kernel serve as they are.
//
// embed_half_scan_kernel<kDimT, kStorage> is embed_scan_kernel with 8 stored values per 16-byte load instead of 4: thread t
// loads the uint4 at vector index tile * kEmbedTileVecs + j * kEmbedBlock + t, G = d / 8 consecutive lanes hold one row (G
// divides 64 and kEmbedBlock: a lane's group index and its 8 user values stay in registers), one wave instruction covers
// 32, 16, 8 or 4 rows and a 32 KiB tile 1024, 512, 256 or 128.  A lane holds TWO of the contract's groups of four, 2g' and
// 2g' + 1: it widens its 8 words (fp16: one hardware conversion each, subnormals kept; bf16: a shift or a mask), forms
// p_(2g') and p_(2g'+1) with embed_partial, takes the contract's first level in-lane, t^1_g' = fl(p_(2g') + p_(2g'+1)), and
// log2(G) xor-butterfly steps give the remaining levels in every lane of the group.  G = 2 takes the xor-1 step alone,
// which embed_tree_levels (kGroup >= 4) cannot: embed_half_tree_levels is the level function here.
// Everything after the widening is fp32 with contraction off: every product is an fp32 product of widened values rounded
// on its own, no mixed-precision or packed-half instruction takes part.
// At d = 16 a tile appends up to 1024 candidates, so the list has kCandLimit + 1024 slots (kEmbedHalfCandCap).
#pragma once

#include "embed.hip.h"
#include "mi355rec_embed_half.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kEmbedHalfMaxTileRows = kEmbedTileVecs / 2;   // d = 16: two lanes per row
constexpr int kEmbedHalfCandCap = kCandLimit + kEmbedHalfMaxTileRows;
constexpr int kEmbedHalfCandPerThread = (kEmbedHalfCandCap + kEmbedBlock - 1) / kEmbedBlock;

// W(x) of the low and of the high 16-bit word of w.
template <int kStorage>
__device__ __forceinline__ float embed_half_widen_lo(uint32_t w) {
    if constexpr (kStorage == MI355REC_EMBED_HALF_FP16) {
        return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w & 0xffffu)));
    } else {
        return __uint_as_float(w << 16);
    }
}
template <int kStorage>
__device__ __forceinline__ float embed_half_widen_hi(uint32_t w) {
    if constexpr (kStorage == MI355REC_EMBED_HALF_FP16) {
        return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w >> 16)));
    } else {
        return __uint_as_float(w & 0xffff0000u);
    }
}

// The 8 stored values of one 16-byte load as the contract's two groups of four.
template <int kStorage>
__device__ __forceinline__ void embed_half_widen8(const uint4& w, float4& lo, float4& hi) {
    lo = make_float4(embed_half_widen_lo<kStorage>(w.x), embed_half_widen_hi<kStorage>(w.x), embed_half_widen_lo<kStorage>(w.y),
                     embed_half_widen_hi<kStorage>(w.y));
    hi = make_float4(embed_half_widen_lo<kStorage>(w.z), embed_half_widen_hi<kStorage>(w.z), embed_half_widen_lo<kStorage>(w.w),
                     embed_half_widen_hi<kStorage>(w.w));
}

// The levels of the contract's tree ABOVE the first (taken in-lane) over the kGroup lanes of a row, kGroup from 2 up.
template <int kGroup>
__device__ __forceinline__ float embed_half_tree_levels(float p) {
    p = p + embed_dpp_xor1(p);
    if constexpr (kGroup >= 4) p = p + embed_dpp_xor2(p);
    if constexpr (kGroup >= 8) p = p + embed_dpp_half_mirror(p);
    if constexpr (kGroup >= 16) p = p + embed_dpp_mirror(p);
    return p;
}

// tree(a, b) of the row whose groups 2g' and 2g' + 1 this lane holds.
template <int kGroup>
__device__ __forceinline__ float embed_half_tree(const float4& a_lo, const float4& a_hi, const float4& b_lo, const float4& b_hi) {
    const float p0 = embed_partial(a_lo, b_lo);
    const float p1 = embed_partial(a_hi, b_hi);
    return embed_half_tree_levels<kGroup>(p0 + p1);
}

// u = W(e_(r0)), then u = fl(u + W(e_(rk))) in list order; one thread per element.
__global__ __launch_bounds__(128) void embed_half_user_kernel(const uint16_t* __restrict__ table, int dim, int storage, EmbedMembers m,
                                                              float* __restrict__ user_out) {
    const int j = threadIdx.x;
    if (j >= dim) return;
    float u = 0.0f;
#pragma unroll 1
    for (int i = 0; i < m.k; ++i) {
        const uint32_t w = table[m.rows[i] * dim + j];
        const float e = storage == MI355REC_EMBED_HALF_FP16 ? embed_half_widen_lo<MI355REC_EMBED_HALF_FP16>(w)
                                                            : embed_half_widen_lo<MI355REC_EMBED_HALF_BF16>(w);
        u = i == 0 ? e : u + e;
    }
    user_out[j] = u;
}

// table: n x kDimT 16-bit words of kStorage; the other arguments and both forms are embed_scan_kernel's.
template <int kDimT, int kStorage>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_half_scan_kernel(
    const uint16_t* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ user, const float* __restrict__ audio_s,
    const uint32_t* __restrict__ exclude, EmbedArgs a, uint64_t* __restrict__ block_lists, float* __restrict__ out_v, float* __restrict__ out_c) {
    constexpr int kGroup = kDimT / 8;                        // lanes per row
    constexpr int kTileRows = kEmbedTileVecs / kGroup;
    static_assert(kGroup >= 2 && kGroup <= 16 && 64 % kGroup == 0, "a row lies inside one wave");
    static_assert(kTileRows <= kEmbedHalfMaxTileRows, "a tile appends at most kEmbedHalfMaxTileRows candidates");
    static_assert(kEmbedHalfCandPerThread * kEmbedBlock >= kEmbedHalfCandCap, "compact_candidates reads the whole list");
    __shared__ uint64_t s_cand[kEmbedHalfCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count;
    __shared__ uint32_t s_excl[kEmbedMaxExclude];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = tid & (kGroup - 1);
    const bool selecting = out_v == nullptr;   // uniform
    const int64_t n_vec = n * kGroup;          // n >= 1 (the host launches nothing for an empty table)
    const uint4* const tab4 = reinterpret_cast<const uint4*>(table);
    const int64_t n_tiles = (n_vec + kEmbedTileVecs - 1) / kEmbedTileVecs;

    auto load_tile = [&](int64_t tile, uint4 (&e)[kEmbedVecsPerThread], float (&s)[kEmbedVecsPerThread]) {
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            int64_t v = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            v = v < n_vec ? v : n_vec - 1;   // (a clamped lane's row is never used: rows are whole groups of lanes)
            e[j] = tab4[v];
            s[j] = a.use_audio ? audio_s[v / kGroup] : 0.0f;
        }
    };

    int64_t tile = blockIdx.x;
    uint4 cur_e[kEmbedVecsPerThread];
    float cur_s[kEmbedVecsPerThread];
    if (tile < n_tiles) load_tile(tile, cur_e, cur_s);   // requested before the user vector is

    if (tid == 0) s_count = 0;
    for (int i = tid; i < a.n_exclude; i += kEmbedBlock) s_excl[i] = exclude[i];
    const float4 u_lo = reinterpret_cast<const float4*>(user)[2 * g];
    const float4 u_hi = reinterpret_cast<const float4*>(user)[2 * g + 1];
    const float nu = sqrtf(embed_half_tree<kGroup>(u_lo, u_hi, u_lo, u_hi));
    __syncthreads();

    uint64_t thr = 0;
    int compact_at = 2 * a.topk > 256 ? 2 * a.topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;

    for (; tile < n_tiles; tile += gridDim.x) {   // uniform
        const int64_t next_tile = tile + gridDim.x;
        uint4 next_e[kEmbedVecsPerThread];
        float next_s[kEmbedVecsPerThread];
        load_tile(next_tile < n_tiles ? next_tile : tile, next_e, next_s);   // the next tile is in flight while this one is scored

#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            const int64_t vec = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            const int64_t row = vec / kGroup;
            float4 e_lo, e_hi;
            embed_half_widen8<kStorage>(cur_e[j], e_lo, e_hi);
            const float dot = embed_half_tree<kGroup>(e_lo, e_hi, u_lo, u_hi);
            float c = dot;
            if (a.metric == 0) {   // uniform
                const float nn = embed_half_tree<kGroup>(e_lo, e_hi, e_lo, e_hi);
                const float den = sqrtf(nn) * nu;
                c = 0.0f;
                if (den > 1e-8f) {
                    const float t = dot / den;
                    const float m = (t < 1.0f) ? t : 1.0f;
                    c = (-1.0f < m) ? m : -1.0f;
                }
            }
            float v = a.w_embed * c;
            if (a.use_audio) {
                const float wa = a.w_audio * cur_s[j];
                v = wa + v;
            }
            const bool owner = g == 0 && vec < n_vec;
            if (!selecting) {
                if (owner) {
                    out_v[row] = v;
                    if (out_c) out_c[row] = c;
                }
                continue;
            }
            uint64_t key = 0;
            if (owner && __builtin_isfinite(v)) key = pack_key(v, static_cast<uint32_t>(row_base + row));
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
        if (selecting) {
            // two barriers: every wave reads the count before any wave appends again (embed_scan_kernel)
            __syncthreads();
            const int c = s_count;
            __syncthreads();
            if (c >= compact_at) {
                const uint64_t local_thr = compact_candidates<kEmbedBlock, kEmbedHalfCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
                if (local_thr > thr) thr = local_thr;
            }
        }
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            cur_e[j] = next_e[j];
            cur_s[j] = next_s[j];
        }
    }
    if (!selecting) return;   // uniform

    __syncthreads();
    if (s_count > kRankCountMax && s_count > a.topk)   // uniform
        compact_candidates<kEmbedBlock, kEmbedHalfCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kEmbedBlock>(s_cand, s_count, block_lists + static_cast<int64_t>(blockIdx.x) * a.topk, a.topk);
}

}  // namespace mi355
