// embed_sets.hip.h — the kernels of libmi355rec_embed_sets.so (gfx950 only): the HYBRID scan RESTRICTED by row sets
// (include/mi355rec_embed_sets.h: a row is admissible iff the plain scan admits it AND its bit of `only AND NOT seen` is
// set).  The scan is embed.hip.h's embed_scan_body under the restriction policy EmbedSetRestriction, over EmbedRowsF32
// and EmbedRowsHalf<fp16 | bf16>; the user kernels, compact_candidates, block_rank_and_store and merge_kernel serve as
// they are.
//
// THE BITMAPS.  Bit i of a uint32 word array is local row i; the host (csrc/embed_sets_request.h) zeroes the bits past
// row n and pads with zero words to a whole number of 32 words, the words of the widest tile.  A tile holds 64 .. 1024 rows,
// a multiple of 32, and starts at a multiple of its rows: it owns kTileWords = 2 .. 32 whole words, tile t the words
// [t * kTileWords, (t + 1) * kTileWords), and no read of a tile t < n_tiles leaves the allocation.  An absent `only` reads
// as all ones, an absent `seen` as zero, and a request with neither reads nothing.
// THE ROW TEST.  A wave instruction covers 64 / G <= 32 rows that start at a multiple of their number: one word.  Each lane
// requests the words of its load's row ahead of the 16-byte load, so they are in flight one tile ahead as audio_s is; the two
// words are carried apart and combined where the row is tested (a combination at the load would wait for the whole tile).
// The bit joins `owner` in the body: a rejected row forms no key, never reaches the candidate list and never runs the
// exclusion list's search; a load in which the wave's ballot shows no admissible row is not scored at all.
// THE TILE SKIP.  A tile whose effective words are all zero is neither loaded nor scored.  next_live(from) is the first live
// tile of from, from + grid, from + 2 grid, ...: every wave reads the same words and derives the same answer, so the decision
// is workgroup-uniform (two barriers follow every scored tile).  The lanes first test the words of `from` together (the dense
// case: one 128-byte line); only if that tile is dead does lane l test the tile from + (l + 1) grid on its own, 64 tiles of
// the stride per round, and the ballot's lowest lane names the tile.  The body's look-ahead load goes to that tile, so the
// double buffer is never spent on a tile that will be dropped.  Each workgroup adds its scored tiles once, at its end, to a
// device counter that the host reads back with the keys.
#pragma once

#include "embed_half.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

struct EmbedSetRestriction {
    static constexpr bool kRestricted = true;
    const uint32_t* only;                // null: every row
    const uint32_t* seen;                // null: no row
    unsigned long long* tiles_scored;    // cumulative

    __device__ __forceinline__ void load_words(int64_t wi, uint32_t& o, uint32_t& s) const {
        o = only ? only[wi] : ~0u;   // uniform
        s = seen ? seen[wi] : 0u;
    }
    __device__ __forceinline__ uint32_t effective(int64_t wi) const {
        uint32_t o, s;
        load_words(wi, o, s);
        return o & ~s;
    }

    // The first live tile of from, from + gridDim.x, ...; n_tiles or more when none is.  The same in every lane of every wave.
    template <int kTileWords>
    __device__ __forceinline__ int64_t next_live(int64_t from, int64_t n_tiles, int lane) const {
        static_assert(kTileWords >= 2 && kTileWords <= 32, "a tile owns 2 to 32 words");
        if (from >= n_tiles || (!only && !seen)) return from;   // uniform
        const uint32_t first = lane < kTileWords ? effective(from * kTileWords + lane) : 0u;
        if (__ballot(first != 0u)) return from;
        const int64_t grid = gridDim.x;
        for (int64_t base = from + grid; base < n_tiles; base += 64 * grid) {   // uniform
            const int64_t cand = base + lane * grid;
            uint32_t any = 0u;
            if (cand < n_tiles) {
#pragma unroll 4
                for (int w = 0; w < kTileWords; ++w) any |= effective(cand * kTileWords + w);
            }
            const uint64_t live = __ballot(any != 0u);
            if (live) return base + static_cast<int64_t>(__ffsll(static_cast<unsigned long long>(live)) - 1) * grid;
        }
        return n_tiles;
    }

    __device__ __forceinline__ void count_scored(int scored) const {
        if (threadIdx.x == 0 && scored > 0) atomicAdd(tiles_scored, static_cast<unsigned long long>(scored));
    }
};

// table: n x kDimT values of Rows; only / seen: the bitmaps or null; the other arguments are embed_scan_body's selecting form.
template <class Rows, int kDimT>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_sets_scan_kernel(
    const typename Rows::Word* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ user, const float* __restrict__ audio_s,
    const uint32_t* __restrict__ exclude, EmbedArgs a, uint64_t* __restrict__ block_lists, const uint32_t* __restrict__ only,
    const uint32_t* __restrict__ seen, unsigned long long* __restrict__ tiles_scored) {
    embed_scan_body<Rows, kDimT, EmbedSetRestriction>(table, n, row_base, user, audio_s, exclude, a, block_lists, nullptr, nullptr,
                                                      EmbedSetRestriction{only, seen, tiles_scored});
}

}  // namespace mi355
