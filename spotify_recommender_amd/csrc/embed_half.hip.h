// embed_half.hip.h — the kernels of libmi355rec_embed_half.so (gfx950 only): the HYBRID scan over a HALF-PRECISION
// embedding table (include/mi355rec_embed_half.h: fp16 or bf16 words, answers those of mi355rec_embed.h's arithmetic
// contract over the widened values W(x), bit for bit) and the kernel that forms a user vector from member rows.
// The scan is embed.hip.h's embed_scan_body over the layout EmbedRowsHalf<kStorage>; embed_probe_kernel (raw 16-byte
// vectors: it reads a half table as it reads an fp32 one) and merge_kernel serve as they are.
//
// EmbedRowsHalf has 8 stored values per 16-byte load instead of 4: thread t loads the uint4 at vector index
// tile * kEmbedTileVecs + j * kEmbedBlock + t, G = d / 8 consecutive lanes hold one row (G
// divides 64 and kEmbedBlock: a lane's group index and its 8 user values stay in registers), one wave instruction covers
// 32, 16, 8 or 4 rows and a 32 KiB tile 1024, 512, 256 or 128.  A lane holds TWO of the contract's groups of four, 2g' and
// 2g' + 1: it widens its 8 words (fp16: one hardware conversion each, subnormals kept; bf16: a shift or a mask), forms
// p_(2g') and p_(2g'+1) with embed_partial, takes the contract's first level in-lane, t^1_g' = fl(p_(2g') + p_(2g'+1)), and
// the log2(G) xor-butterfly steps of embed_tree_levels<G> give the remaining levels in every lane of the group (G = 2, at
// d = 16, takes the xor-1 step alone).
// Everything after the widening is fp32 with contraction off: every product is an fp32 product of widened values rounded
// on its own, no mixed-precision or packed-half instruction takes part.
// At d = 16 a tile appends up to 1024 candidates, so the body's list has kCandLimit + 1024 slots.
#pragma once

#include "embed.hip.h"
#include "mi355rec_embed_half.h"

#pragma clang fp contract(off)

namespace mi355 {

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

// The half row layout: eight stored values per 16-byte load, the contract's groups of four 2g' and 2g' + 1 per lane.
struct EmbedRow8 {
    float4 lo, hi;
};
template <int kStorage>
struct EmbedRowsHalf {
    using Word = uint16_t;
    using Vec = uint4;
    using Row = EmbedRow8;
    static constexpr int kVals = 8;
    static __device__ __forceinline__ Row widen(const Vec& w) {
        Row r;
        embed_half_widen8<kStorage>(w, r.lo, r.hi);
        return r;
    }
    static __device__ __forceinline__ Row user(const float* u, int g) {
        return {reinterpret_cast<const float4*>(u)[2 * g], reinterpret_cast<const float4*>(u)[2 * g + 1]};
    }
    // p_(2g') and p_(2g'+1), then the contract's first level in-lane
    static __device__ __forceinline__ float partial(const Row& a, const Row& b) {
        const float p0 = embed_partial(a.lo, b.lo);
        const float p1 = embed_partial(a.hi, b.hi);
        return p0 + p1;
    }
};

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

// table: n x kDimT 16-bit words of kStorage; the other arguments and both forms are embed_scan_body's.
template <int kDimT, int kStorage>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_half_scan_kernel(
    const uint16_t* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ user, const float* __restrict__ audio_s,
    const uint32_t* __restrict__ exclude, EmbedArgs a, uint64_t* __restrict__ block_lists, float* __restrict__ out_v, float* __restrict__ out_c) {
    embed_scan_body<EmbedRowsHalf<kStorage>, kDimT>(table, n, row_base, user, audio_s, exclude, a, block_lists, out_v, out_c);
}

}  // namespace mi355
