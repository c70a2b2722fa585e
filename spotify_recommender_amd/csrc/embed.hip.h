// embed.hip.h — the kernels of libmi355rec_embed.so (gfx950 only): the HYBRID scan over an embedding table
// (include/mi355rec_embed.h has the arithmetic contract), the kernel that forms a user vector from member rows, and the
// plain read of the table that the scan is measured against.
//
// embed_scan_body<Rows, kDimT> is the scan, written once: embed_scan_kernel<kDimT> here and embed_half_scan_kernel
// (embed_half.hip.h) are one call of it each.  Rows is the layout of a stored row: Word (the table's element), Vec (the
// 16-byte load), kVals (stored values per load), Row (the widened values a lane holds), widen(Vec) -> Row,
// user(u, g) -> Row (lane g's values of the user vector) and partial(Row, Row) -> float (the lane's part of the contract's
// tree).  EmbedRowsF32 below is the fp32 layout (kVals = 4, one group of four per lane); the body derives its lanes per row,
// its widest tile and its candidate list's capacity from kVals.
//
// The body streams the table (n x d, row-major) with 16-byte loads: thread t of a workgroup loads the
// Vec at vector index tile * kTileVecs + j * kBlock + t, so every wave instruction reads 1 KiB of consecutive bytes.
// G = d / kVals consecutive lanes hold one row (G divides 64 and kBlock, so a lane's group index g = t % G never changes and
// its user values stay in registers): each lane forms its partial p_g of the dot product and of the row's squared
// norm, and log2(G) xor-butterfly steps leave the contract's tree sum in EVERY lane of the group — fl(a + b) is symmetric,
// so the butterfly's t(l+1) = fl(t_g + t_(g xor 2^l)) is the contract's fl(t_(2g) + t_(2g+1)).  One fp32 wave instruction
// thus covers 16, 8, 4 or 2 rows.  Steps 1 and 2 are quad permutes, 4 and 8 the half-row and row mirrors of DPP (after the
// steps before them all lanes they could pick hold one value), 16 a ds_bpermute.
// s(x), the audio cosine, is read at 4 B per row from the vector mi355rec_enqueue_scores wrote (w_audio != 0 only).
// Two tiles of kEmbedVecsPerThread loads each are in flight per lane (the tile being scored and the next one, in registers:
// 64 KiB per workgroup), and two workgroups of 512 threads share a CU (__launch_bounds__(512, 4): at most 128 VGPRs).
// The lane with g == 0 forms the key; candidates, thresholds and the per-workgroup lists are core.hip.h's pieces used as
// label_scan_kernel uses them (no launch-wide bound, no pre-filter: DESIGN.md §5.4.21); merge_kernel (merge.hip.h) follows.
// With out_v the launch is the parity hook instead: v (and c) of every row are stored and nothing is selected.
//
// The body takes a compile-time RESTRICTION POLICY (default EmbedNoRestriction: the plain scan, which reads and holds
// nothing more).  A restricting policy (embed_sets.hip.h) names the tiles the workgroup scores (next_live), the bitmap
// words a tile's rows are tested against (loaded with the tile, one tile ahead) and the row test that joins `owner`.
#pragma once

#include "core.hip.h"
#include "merge.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kEmbedBlock = 512;
constexpr int kEmbedVecsPerThread = 4;                            // 16-byte loads per lane per tile
constexpr int kEmbedTileVecs = kEmbedBlock * kEmbedVecsPerThread;   // 32 KiB per tile
constexpr int kEmbedMaxExclude = 1024;
constexpr int kEmbedMaxMembers = 32;

struct EmbedArgs {
    float w_audio;
    float w_embed;
    int metric;      // 0 cosine, 1 dot
    int use_audio;
    int n_exclude;   // sorted, distinct LOCAL rows in `exclude`
    int topk;
};

struct EmbedMembers {
    int64_t rows[kEmbedMaxMembers];
    int k;
};

__device__ __forceinline__ float embed_dpp_xor1(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));   // quad_perm:[1,0,3,2]
}
__device__ __forceinline__ float embed_dpp_xor2(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));   // quad_perm:[2,3,0,1]
}
__device__ __forceinline__ float embed_dpp_half_mirror(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xf, 0xf, true));  // row_half_mirror
}
__device__ __forceinline__ float embed_dpp_mirror(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xf, 0xf, true));   // row_mirror
}

// The levels of the contract's tree over the kGroup lanes of a row (2 to 32); the sum ends in every lane of the group.
template <int kGroup>
__device__ __forceinline__ float embed_tree_levels(float p) {
    p = p + embed_dpp_xor1(p);
    if constexpr (kGroup >= 4) p = p + embed_dpp_xor2(p);
    if constexpr (kGroup >= 8) p = p + embed_dpp_half_mirror(p);
    if constexpr (kGroup >= 16) p = p + embed_dpp_mirror(p);
    if constexpr (kGroup >= 32) p = p + __shfl_xor(p, 16, 64);
    return p;
}

// The group partial of four: fl(fl(fl(a0 b0 + a1 b1) + a2 b2) + a3 b3), every product rounded on its own.
__device__ __forceinline__ float embed_partial(const float4& a, const float4& b) {
    float p = a.x * b.x;
    p = p + a.y * b.y;
    p = p + a.z * b.z;
    p = p + a.w * b.w;
    return p;
}

// u = e_(r0), then u = fl(u + e_(rk)) in list order; one thread per element.
__global__ __launch_bounds__(128) void embed_user_kernel(const float* __restrict__ table, int dim, EmbedMembers m,
                                                                                    float* __restrict__ user_out) {
    const int j = threadIdx.x;
    if (j >= dim) return;
    float u = 0.0f;
#pragma unroll 1
    for (int i = 0; i < m.k; ++i) {
        const float e = table[m.rows[i] * dim + j];
        u = i == 0 ? e : u + e;
    }
    user_out[j] = u;
}

// A plain read of n_vec 16-byte vectors (the ceiling the scan is held against); one checksum word per workgroup.
__global__ __launch_bounds__(kEmbedBlock) void embed_probe_kernel(const float4* __restrict__ buf, int64_t n_vec, uint32_t* __restrict__ sink) {
    uint32_t acc = 0;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kEmbedBlock;
    int64_t i = static_cast<int64_t>(blockIdx.x) * kEmbedBlock + threadIdx.x;
    for (; i + 3 * stride < n_vec; i += 4 * stride) {
        const float4 a = buf[i], b = buf[i + stride], c = buf[i + 2 * stride], d = buf[i + 3 * stride];
        acc += __float_as_uint(a.x) ^ __float_as_uint(b.y) ^ __float_as_uint(c.z) ^ __float_as_uint(d.w);
    }
    for (; i < n_vec; i += stride) acc += __float_as_uint(buf[i].x);
    acc = wave_max_u32(acc);
    __shared__ uint32_t s_acc;
    if (threadIdx.x == 0) s_acc = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_acc, acc);
    __syncthreads();
    if (threadIdx.x == 0) sink[blockIdx.x] = s_acc;
}

// The fp32 row layout: four stored values per 16-byte load, one group of four per lane.
struct EmbedRowsF32 {
    using Word = float;
    using Vec = float4;
    using Row = float4;
    static constexpr int kVals = 4;
    static __device__ __forceinline__ Row widen(const Vec& w) { return w; }
    static __device__ __forceinline__ Row user(const float* u, int g) { return reinterpret_cast<const float4*>(u)[g]; }
    static __device__ __forceinline__ float partial(const Row& a, const Row& b) { return embed_partial(a, b); }
};

// The policy of the plain scan: every tile of the workgroup's stride is live and every row passes.
struct EmbedNoRestriction {
    static constexpr bool kRestricted = false;
    template <int kTileWords>
    __device__ __forceinline__ int64_t next_live(int64_t from, int64_t, int) const { return from; }
};

// The scan over a table of n x kDimT Rows::Word (the one body of embed_scan_kernel and embed_half_scan_kernel).
// user: kDimT floats (device); audio_s: n floats or null (use_audio == 0); exclude: n_exclude sorted local rows.
// Selecting form (out_v == null): block_lists[gridDim.x][topk].  Scoring form: out_v[n], out_c[n] or null.
template <class Rows, int kDimT, class Restrict = EmbedNoRestriction>
__device__ __forceinline__ void embed_scan_body(const typename Rows::Word* __restrict__ table, int64_t n, int64_t row_base,
                                                const float* __restrict__ user, const float* __restrict__ audio_s,
                                                const uint32_t* __restrict__ exclude, EmbedArgs a, uint64_t* __restrict__ block_lists,
                                                float* __restrict__ out_v, float* __restrict__ out_c, const Restrict rs = Restrict{}) {
    using Vec = typename Rows::Vec;
    using Row = typename Rows::Row;
    constexpr int kGroup = kDimT / Rows::kVals;                        // lanes per row
    constexpr int kTileRows = kEmbedTileVecs / kGroup;
    constexpr int kMaxTileRows = kEmbedTileVecs / (16 / Rows::kVals);   // d = 16
    constexpr int kCandCap = kCandLimit + kMaxTileRows;
    constexpr int kCandPerThread = (kCandCap + kEmbedBlock - 1) / kEmbedBlock;
    constexpr int kTileWords = kTileRows / 32;                         // bitmap words of a tile (a restricting policy's)
    constexpr int kSetWords = Restrict::kRestricted ? kEmbedVecsPerThread : 1;
    static_assert(kTileRows % 32 == 0 && kTileWords >= 2, "a tile owns whole bitmap words");
    static_assert(kGroup >= 2 && kGroup <= 32 && 64 % kGroup == 0, "a row lies inside one wave");
    static_assert(kTileRows <= kMaxTileRows, "a tile appends at most kMaxTileRows candidates");
    static_assert(kCandPerThread * kEmbedBlock >= kCandCap, "compact_candidates reads the whole list");
    __shared__ uint64_t s_cand[kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count;
    __shared__ uint32_t s_excl[kEmbedMaxExclude];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = tid & (kGroup - 1);
    const bool selecting = out_v == nullptr;   // uniform
    const int64_t n_vec = n * kGroup;          // n >= 1 (the host launches nothing for an empty table)
    const Vec* const tab4 = reinterpret_cast<const Vec*>(table);
    const int64_t n_tiles = (n_vec + kEmbedTileVecs - 1) / kEmbedTileVecs;

    auto load_tile = [&](int64_t tile, Vec (&e)[kEmbedVecsPerThread], float (&s)[kEmbedVecsPerThread], uint32_t (&wo)[kSetWords],
                         uint32_t (&ws)[kSetWords]) {
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            int64_t v = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            v = v < n_vec ? v : n_vec - 1;   // (a clamped lane's row is never used: rows are whole groups of lanes)
            if constexpr (Restrict::kRestricted) rs.load_words((v / kGroup) >> 5, wo[j], ws[j]);   // (ahead of the 16-byte load)
            e[j] = tab4[v];
            s[j] = a.use_audio ? audio_s[v / kGroup] : 0.0f;
        }
    };
    auto tree = [](const Row& x, const Row& y) { return embed_tree_levels<kGroup>(Rows::partial(x, y)); };

    int64_t tile = rs.template next_live<kTileWords>(blockIdx.x, n_tiles, lane);   // uniform
    Vec cur_e[kEmbedVecsPerThread];
    float cur_s[kEmbedVecsPerThread];
    uint32_t cur_wo[kSetWords], cur_ws[kSetWords];
    if (tile < n_tiles) load_tile(tile, cur_e, cur_s, cur_wo, cur_ws);   // requested before the user vector is

    if (tid == 0) s_count = 0;
    for (int i = tid; i < a.n_exclude; i += kEmbedBlock) s_excl[i] = exclude[i];
    const Row u = Rows::user(user, g);
    const float nu = sqrtf(tree(u, u));
    __syncthreads();

    uint64_t thr = 0;
    int compact_at = 2 * a.topk > 256 ? 2 * a.topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;

    int scored = 0;
    int64_t next_tile;
    for (; tile < n_tiles; tile = next_tile) {   // uniform
        next_tile = rs.template next_live<kTileWords>(tile + gridDim.x, n_tiles, lane);   // (the plain scan: tile + gridDim.x)
        Vec next_e[kEmbedVecsPerThread];
        float next_s[kEmbedVecsPerThread];
        uint32_t next_wo[kSetWords], next_ws[kSetWords];
        load_tile(next_tile < n_tiles ? next_tile : tile, next_e, next_s, next_wo, next_ws);   // the next tile is in flight while this one is scored
        if constexpr (Restrict::kRestricted) ++scored;

#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            const int64_t vec = tile * kEmbedTileVecs + j * kEmbedBlock + tid;
            const int64_t row = vec / kGroup;
            bool admitted = true;
            if constexpr (Restrict::kRestricted) {
                // the row's bit joins owner: a rejected row forms no key; a load with no admissible row in the wave is not scored
                admitted = (((cur_wo[j] & ~cur_ws[j]) >> (static_cast<uint32_t>(row) & 31u)) & 1u) != 0u;
                if (!__ballot(admitted && g == 0 && vec < n_vec)) continue;   // (wave-uniform: the butterflies stay inside the wave)
            }
            const Row e = Rows::widen(cur_e[j]);
            const float dot = tree(e, u);
            float c = dot;
            if (a.metric == 0) {   // uniform
                const float nn = tree(e, e);
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
            const bool owner = g == 0 && vec < n_vec && admitted;
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
            // two barriers: every wave reads the count before any wave appends again (scan_kernel)
            __syncthreads();
            const int c = s_count;
            __syncthreads();
            if (c >= compact_at) {
                const uint64_t local_thr = compact_candidates<kEmbedBlock, kCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
                if (local_thr > thr) thr = local_thr;
            }
        }
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            cur_e[j] = next_e[j];
            cur_s[j] = next_s[j];
            if constexpr (Restrict::kRestricted) {
                cur_wo[j] = next_wo[j];
                cur_ws[j] = next_ws[j];
            }
        }
    }
    if (!selecting) return;   // uniform
    if constexpr (Restrict::kRestricted) rs.count_scored(scored);   // once per workgroup

    __syncthreads();
    if (s_count > kRankCountMax && s_count > a.topk)   // uniform
        compact_candidates<kEmbedBlock, kCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kEmbedBlock>(s_cand, s_count, block_lists + static_cast<int64_t>(blockIdx.x) * a.topk, a.topk);
}

// table: n x kDimT floats; the other arguments and both forms are embed_scan_body's.
template <int kDimT>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_scan_kernel(
    const float* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ user, const float* __restrict__ audio_s,
    const uint32_t* __restrict__ exclude, EmbedArgs a, uint64_t* __restrict__ block_lists, float* __restrict__ out_v, float* __restrict__ out_c) {
    embed_scan_body<EmbedRowsF32, kDimT>(table, n, row_base, user, audio_s, exclude, a, block_lists, out_v, out_c);
}

}  // namespace mi355
