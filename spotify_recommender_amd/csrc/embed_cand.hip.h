// embed_cand.hip.h — the kernels of libmi355rec_embed_cand.so (gfx950 only; include/mi355rec_embed_cand.h).
//
// embed_cand_kernel<Rows, kDimT> is embed_scan_body (embed.hip.h) with the tile's vector index replaced by a list lookup.
// A tile is kEmbedTileVecs 16-byte slots as there, so kTileEntries = kEmbedTileVecs / G list entries (G = kDimT / kVals
// lanes per row: the scan's tile rows): slot j * kEmbedBlock + t of a tile belongs to entry slot / G, and the G consecutive
// lanes of a group read the SAME list word (one address per group: a broadcast load), then the row's 16-byte vector
// row * G + g.  A wave instruction thus reads 64 / G segments of 16 G bytes — 32 B (fp16, d = 16) to 512 B (fp32, d = 128)
// of consecutive bytes each, from rows that lie anywhere.  Everything after the load is the contract's arithmetic through
// the scan's own pieces (Rows::widen / user / partial, embed_tree_levels<G>, the cosine clamp and the blend with
// contraction off, pack_key, the LDS exclusion search, compact_candidates, block_rank_and_store), merge_kernel and
// embed_stream_finish_kernel behind it.
//
// THE DEPENDENT LOADS.  A row's address is a loaded value, so a tile's chain is two misses long.  Three tiles are in
// flight per lane: the list words of tile k + 2 are requested while the rows of tile k + 1 are (their words arrived while
// tile k - 1 was scored) and while tile k is scored.  That is 4 + 4 + 4 list words and 2 x 4 row vectors in registers.
//
// NO BRANCH AROUND THE TREE.  An entry past the list's end, an id outside the table and an unclaimed duplicate all carry
// the no-row word kEmbedStreamNoRow.  Such a lane's LOAD is predicated off (its vector is zero: c = 0, no NaN is made up),
// but the lane walks through every DPP butterfly with its wave; it is `owner` that keeps it from forming a key (selecting
// form) and the NaN rule that fills its value (scoring form).
//
// The two forms, under one uniform flag as in embed_scan_body.  SELECTING (out_v == null): `rows` is the claimed list
// embed_cand_claim_kernel wrote (local rows, kEmbedStreamNoRow for whatever forms no key), block_lists[gridDim.x][topk] is
// written, and every owner stores 0 over the word of the claim bitmap that holds its bit: the claims were all made by the
// launch before this one and every set bit has exactly one owner, so plain stores of 0 — idempotent, from whichever owners
// share a word — leave the bitmap all zero for the next call in stream order.  SCORING: `rows` is null, the ids are
// mapped here, nothing is claimed, and v, c and the flag of every entry are stored in list order.
//
// embed_cand_claim_kernel maps id i to its local row (embed_stream_prepare_kernel's rule) and claims the row's bit with
// atomicOr; the entry that finds the bit set is a duplicate and becomes the no-row word.  Which copy of a row wins varies
// from run to run; the key it forms does not (the same row, the same v), so the answer is deterministic.
#pragma once

#include "embed_stream.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kEmbedCandMax = 1 << 20;      // MI355REC_EMBED_CAND_MAX
constexpr int kEmbedCandClaimBlock = 256;
constexpr int kEmbedCandClaimGrid = 1024;   // the most workgroups of a claim launch (2^20 entries: four per thread)

// A global id as a local row of a table of n rows from row_base on, or the no-row word (compared before the subtraction).
__device__ __forceinline__ uint32_t embed_cand_local_row(int64_t id, int64_t row_base, int64_t n) {
    return (id >= 0 && id >= row_base && id - row_base < n) ? static_cast<uint32_t>(id - row_base) : kEmbedStreamNoRow;
}

// ids: m global ids; claim: (n + 31) / 32 words, all zero on entry; rows_out: m words.
__global__ __launch_bounds__(kEmbedCandClaimBlock) void embed_cand_claim_kernel(const int64_t* __restrict__ ids, int64_t m, int64_t row_base, int64_t n,
                                                                                uint32_t* __restrict__ claim, uint32_t* __restrict__ rows_out) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kEmbedCandClaimBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kEmbedCandClaimBlock + threadIdx.x; i < m; i += stride) {
        uint32_t local = embed_cand_local_row(ids[i], row_base, n);
        if (local != kEmbedStreamNoRow) {
            const uint32_t bit = 1u << (local & 31u);
            if (atomicOr(&claim[local >> 5], bit) & bit) local = kEmbedStreamNoRow;
        }
        rows_out[i] = local;
    }
}

// table: n x kDimT Rows::Word (n may be 0 in the scoring form: no row is read then); m >= 1 list entries, as `rows` (the
// claimed local rows: selecting form) or as `ids` (global ids: scoring form).  user, audio_s (indexed by local row),
// exclude and a are embed_scan_body's.  Selecting: block_lists[gridDim.x][topk], claim as above.  Scoring: out_v[m],
// out_c[m] or null, out_flag[m] or null.  gridDim.x <= the tiles of the list.
template <class Rows, int kDimT>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_cand_kernel(
    const typename Rows::Word* __restrict__ table, int64_t n, int64_t row_base, const int64_t* __restrict__ ids, const uint32_t* __restrict__ rows,
    int64_t m, const float* __restrict__ user, const float* __restrict__ audio_s, const uint32_t* __restrict__ exclude, EmbedArgs a,
    uint64_t* __restrict__ block_lists, uint32_t* __restrict__ claim, float* __restrict__ out_v, float* __restrict__ out_c,
    uint8_t* __restrict__ out_flag) {
    using Vec = typename Rows::Vec;
    using Row = typename Rows::Row;
    constexpr int kGroup = kDimT / Rows::kVals;                        // lanes per row
    constexpr int kTileEntries = kEmbedTileVecs / kGroup;
    constexpr int kMaxTileRows = kEmbedTileVecs / (16 / Rows::kVals);   // d = 16
    constexpr int kCandCap = kCandLimit + kMaxTileRows;
    constexpr int kCandPerThread = (kCandCap + kEmbedBlock - 1) / kEmbedBlock;
    static_assert(kGroup >= 2 && kGroup <= 32 && 64 % kGroup == 0, "a row lies inside one wave");
    static_assert(kTileEntries <= kMaxTileRows, "a tile appends at most kMaxTileRows candidates");
    static_assert(kCandPerThread * kEmbedBlock >= kCandCap, "compact_candidates reads the whole list");
    __shared__ uint64_t s_cand[kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count;
    __shared__ uint32_t s_excl[kEmbedMaxExclude];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = tid & (kGroup - 1);
    const bool selecting = out_v == nullptr;   // uniform
    const Vec* const tab4 = reinterpret_cast<const Vec*>(table);
    const int64_t n_tiles = (m + kTileEntries - 1) / kTileEntries;

    // the list words of a tile (any tile: an entry from m on is the no-row word and reads nothing)
    auto load_list = [&](int64_t tile, uint32_t (&r)[kEmbedVecsPerThread]) {
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            const int64_t entry = tile * kTileEntries + (j * kEmbedBlock + tid) / kGroup;
            uint32_t row = kEmbedStreamNoRow;
            if (entry < m) row = rows ? rows[entry] : embed_cand_local_row(ids[entry], row_base, n);
            r[j] = row;
        }
    };
    // ... and the rows they name
    auto load_rows = [&](const uint32_t (&r)[kEmbedVecsPerThread], Vec (&e)[kEmbedVecsPerThread], float (&s)[kEmbedVecsPerThread]) {
#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            Vec w;
            w.x = w.y = w.z = w.w = 0;
            float sa = 0.0f;
            if (r[j] != kEmbedStreamNoRow) {   // (a row < n: the only addresses formed)
                w = tab4[static_cast<int64_t>(r[j]) * kGroup + g];
                if (a.use_audio) sa = audio_s[r[j]];
            }
            e[j] = w;
            s[j] = sa;
        }
    };
    auto tree = [](const Row& x, const Row& y) { return embed_tree_levels<kGroup>(Rows::partial(x, y)); };

    int64_t tile = blockIdx.x;   // < n_tiles
    uint32_t cur_r[kEmbedVecsPerThread], next_r[kEmbedVecsPerThread];
    Vec cur_e[kEmbedVecsPerThread];
    float cur_s[kEmbedVecsPerThread];
    load_list(tile, cur_r);
    load_list(tile + gridDim.x, next_r);
    load_rows(cur_r, cur_e, cur_s);   // requested before the user vector is

    if (tid == 0) s_count = 0;
    for (int i = tid; i < a.n_exclude; i += kEmbedBlock) s_excl[i] = exclude[i];
    const Row u = Rows::user(user, g);
    const float nu = sqrtf(tree(u, u));
    __syncthreads();

    uint64_t thr = 0;
    int compact_at = 2 * a.topk > 256 ? 2 * a.topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;
    const float quiet_nan = __uint_as_float(0x7FC00000u);

    for (; tile < n_tiles; tile += gridDim.x) {   // uniform
        Vec next_e[kEmbedVecsPerThread];
        float next_s[kEmbedVecsPerThread];
        uint32_t far_r[kEmbedVecsPerThread];
        load_rows(next_r, next_e, next_s);                               // the next tile's rows are in flight while this one is scored,
        load_list(tile + 2 * static_cast<int64_t>(gridDim.x), far_r);   // and the list words of the tile after it

#pragma unroll
        for (int j = 0; j < kEmbedVecsPerThread; ++j) {
            const uint32_t row = cur_r[j];
            const Row e = Rows::widen(cur_e[j]);
            const float dot = tree(e, u);
            float c = dot;
            if (a.metric == 0) {   // uniform
                const float nn = tree(e, e);
                const float den = sqrtf(nn) * nu;
                c = 0.0f;
                if (den > 1e-8f) {
                    const float t = dot / den;
                    const float mm = (t < 1.0f) ? t : 1.0f;
                    c = (-1.0f < mm) ? mm : -1.0f;
                }
            }
            float v = a.w_embed * c;
            if (a.use_audio) {
                const float wa = a.w_audio * cur_s[j];
                v = wa + v;
            }
            const bool owner = g == 0 && row != kEmbedStreamNoRow;
            if (!selecting) {
                const int64_t entry = tile * kTileEntries + (j * kEmbedBlock + tid) / kGroup;
                if (g == 0 && entry < m) {
                    const bool in_table = row != kEmbedStreamNoRow;
                    out_v[entry] = in_table ? v : quiet_nan;
                    if (out_c) out_c[entry] = in_table ? c : quiet_nan;
                    if (out_flag) out_flag[entry] = in_table ? 1 : 0;
                }
                continue;
            }
            uint64_t key = 0;
            if (owner) {
                claim[row >> 5] = 0u;   // (the owner's bit, and its word-mates' whose owners store the same 0)
                if (__builtin_isfinite(v)) key = pack_key(v, static_cast<uint32_t>(row_base + row));
            }
            bool pass = key > thr;
            if (pass && a.n_exclude > 0) {   // (rare once the threshold stands: a binary search over the sorted list in LDS)
                int lo = 0, hi = a.n_exclude;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_excl[mid] < row) lo = mid + 1;
                    else hi = mid;
                }
                pass = !(lo < a.n_exclude && s_excl[lo] == row);
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
            cur_r[j] = next_r[j];
            next_r[j] = far_r[j];
        }
    }
    if (!selecting) return;   // uniform

    __syncthreads();
    if (s_count > kRankCountMax && s_count > a.topk)   // uniform
        compact_candidates<kEmbedBlock, kCandPerThread>(s_cand, &s_count, a.topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kEmbedBlock>(s_cand, s_count, block_lists + static_cast<int64_t>(blockIdx.x) * a.topk, a.topk);
}

}  // namespace mi355
