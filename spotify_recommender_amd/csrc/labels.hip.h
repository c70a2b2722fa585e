// labels.hip.h — the LABEL-FILTERED scan (gfx950 only): the top-N rows whose label is in a given set, over the label-grouped
// copy of a shard's rows that mi355rec_set_labels builds (engine_labels.hip.h).
//
// The rows are stored grouped by label (labels ascending, rows stable inside a label, unlabelled rows last), so the rows
// of one label are one contiguous run of 48-B records: a query restricted to a few labels streams those runs and nothing
// else.  Tiles of kTileRows rows never cross a label boundary (a label's last tile is partial); the selected labels'
// tiles, taken in label order, are dealt round-robin over the workgroups (global tile t -> workgroup t % grid), as
// scan_kernel's interleaved mode deals the tiles of the whole shard.  Every workgroup derives that numbering itself from
// the 1024-bit label mask (a kernel argument) and the label offsets on the device; the host only sizes the grid.
//
// Arithmetic, pre-filter and selection are scan_kernel's (kernels.hip.h): cosine_score (the reference's chain, bit for
// bit), the approx_cosine pre-filter under kApproxMargin while the threshold score is positive and |q| < kApproxMaxQueryNorm,
// keys packed with the ORIGINAL global row (so ties break as in every other route), the excluded row dropped by its global
// index, keys at or above *upper dropped (the rounds of topn > 1024), candidates compacted and ranked by
// compact_candidates / block_rank_and_store into block_lists[workgroup][0..topk).  No launch-wide bound: thresholds are
// per workgroup.
#pragma once

#include "core.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kMaxLabels = 1024;   // MI355REC_MAX_LABELS
using LabelScanCfg = ScanCfg<512, 1, 6>;

struct LabelMask {
    uint32_t w[kMaxLabels / 32];   // bit l of w[l / 32]: label l is selected
};

// lab_feats: the shard's rows grouped by label; lab_rows[pos]: the shard-local row of sorted position pos;
// lab_off[l] .. lab_off[l + 1]: the positions of label l (lab_off[kMaxLabels] = where the unlabelled rows start).
// query_ptr != null: the query's 12 floats are read from there (a resident row); else they are qarg.q.
__global__ __launch_bounds__(LabelScanCfg::kBlock, LabelScanCfg::kMinWaves) void label_scan_kernel(
    const float* __restrict__ lab_feats, const uint32_t* __restrict__ lab_rows, const int64_t* __restrict__ lab_off,
    LabelMask mask, int64_t row_base, QueryArg qarg, const float* __restrict__ query_ptr, int64_t exclude_global, int topk,
    uint64_t* __restrict__ block_lists, const uint64_t* __restrict__ upper_ptr) {
    constexpr int kBlock = LabelScanCfg::kBlock;
    constexpr int kTileRows = LabelScanCfg::kTileRows;
    static_assert(LabelScanCfg::kRowsPerThread == 1 && kTileRows == kBlock, "one row per lane per tile");
    static_assert(kMaxLabels == 2 * kBlock, "two labels per thread in the tile numbering");
    __shared__ uint64_t s_cand[LabelScanCfg::kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count;
    __shared__ uint32_t s_tile0[kMaxLabels + 1];   // global number of label l's first tile; [kMaxLabels] = all tiles
    __shared__ int64_t s_off[kMaxLabels + 1];      // lab_off, so that a tile's rows are found without a global load
    __shared__ int s_wave_sum[kBlock / 64];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // ---- the tile numbering: tiles of the selected labels, in label order (thread t: labels 2t, 2t + 1) ----
    {
        const int l0 = 2 * tid, l1 = 2 * tid + 1;
        const int64_t o0 = lab_off[l0], o1 = lab_off[l1], o2 = lab_off[l1 + 1];
        uint32_t word = 0;   // mask.w[tid / 16], selected without a dynamic index into the kernel argument
#pragma unroll
        for (int w = 0; w < kMaxLabels / 32; ++w) word = w == (tid >> 4) ? mask.w[w] : word;
        const bool sel0 = (word >> (l0 & 31)) & 1u, sel1 = (word >> (l1 & 31)) & 1u;
        const int c0 = sel0 ? static_cast<int>((o1 - o0 + kTileRows - 1) / kTileRows) : 0;
        const int c1 = sel1 ? static_cast<int>((o2 - o1 + kTileRows - 1) / kTileRows) : 0;
        const int incl = wave_inclusive_scan(c0 + c1);
        if (lane == 63) s_wave_sum[wave] = incl;
        if (tid == 0) s_count = 0;
        __syncthreads();
        int before = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) before += w < wave ? s_wave_sum[w] : 0;
        const int excl = before + incl - (c0 + c1);
        s_tile0[l0] = static_cast<uint32_t>(excl);
        s_tile0[l1] = static_cast<uint32_t>(excl + c0);
        s_off[l0] = o0;
        s_off[l1] = o1;
        if (tid == kBlock - 1) {
            s_tile0[kMaxLabels] = static_cast<uint32_t>(excl + c0 + c1);
            s_off[kMaxLabels] = o2;
        }
        __syncthreads();
    }
    const uint32_t n_tiles = s_tile0[kMaxLabels];
    // rows [begin, end) of global tile t (t < n_tiles): the label is the last one whose first tile is <= t (labels without
    // tiles share their successor's number, so the search lands on the one that has it)
    auto tile_rows = [&](uint32_t t, int64_t& begin, int64_t& end) {
        int lo = 0, hi = kMaxLabels - 1;
        while (lo < hi) {   // (uniform: every lane searches for the same t)
            const int mid = (lo + hi + 1) >> 1;
            if (s_tile0[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        begin = s_off[lo] + static_cast<int64_t>(t - s_tile0[lo]) * kTileRows;
        end = s_off[lo + 1];
        if (end > begin + kTileRows) end = begin + kTileRows;
    };

    const uint32_t stride = gridDim.x;
    uint32_t t = blockIdx.x;
    // the first tile is requested before the query is (scan_kernel does the same: the query sits behind dependent loads)
    int64_t cur_begin = 0, cur_end = 1;
    if (t < n_tiles) tile_rows(t, cur_begin, cur_end);
    const int64_t r0 = cur_begin + tid;
    Row cur = load_row(lab_feats, r0 < cur_end ? r0 : cur_end - 1);

    float q[kDim];
    if (query_ptr) {   // (uniform: one instantiation for both kinds of query)
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = query_ptr[j];
    } else {
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = qarg.q[j];
    }
    const float qn = query_norm(q);
    const float inv_qn = 1.0f / qn;
    const bool prefilter_ok = qn < kApproxMaxQueryNorm;   // false for inf / NaN norms too
    const uint64_t upper = upper_ptr ? *upper_ptr : ~0ull;
    uint64_t thr = 0;
    float cutoff = 0.0f;   // the pre-filter is active only while > 0
    int compact_at = 2 * topk > 256 ? 2 * topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;

    for (; t < n_tiles; t += stride) {   // uniform
        // the next tile's rows are in flight while this one is scored
        const uint32_t tn = t + stride;
        int64_t nb = cur_begin, ne = cur_end;
        if (tn < n_tiles) tile_rows(tn, nb, ne);
        const int64_t rn = nb + tid;
        const Row next = load_row(lab_feats, rn < ne ? rn : ne - 1);

        const int64_t pos = cur_begin + tid;
        const bool in_range = pos < cur_end;
        bool maybe = in_range;
        if (cutoff > 0.0f) maybe = maybe && !(approx_cosine(q, inv_qn, cur) < cutoff);
        if (__ballot(maybe)) {
            const float s = cosine_score(q, qn, cur);
            const int64_t g = maybe ? row_base + static_cast<int64_t>(lab_rows[pos]) : -1;   // the id only where it can matter
            uint64_t key = pack_key(s, static_cast<uint32_t>(g));
            if (!maybe || g == exclude_global || key >= upper) key = 0;
            const bool pass = key > thr;
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
            const uint64_t local_thr = compact_candidates<kBlock, LabelScanCfg::kCandPerThread>(s_cand, &s_count, topk, false, s_sel);
            if (local_thr > thr) {
                thr = local_thr;
                if (prefilter_ok) cutoff = ordered_to_score(static_cast<uint32_t>(thr >> 32)) - kApproxMargin;
            }
        }
        cur = next;
        cur_begin = nb;
        cur_end = ne;
    }

    __syncthreads();
    if (s_count > kRankCountMax && s_count > topk)   // uniform
        compact_candidates<kBlock, LabelScanCfg::kCandPerThread>(s_cand, &s_count, topk, false, s_sel);
    __syncthreads();
    block_rank_and_store<kBlock>(s_cand, s_count, block_lists + static_cast<int64_t>(blockIdx.x) * topk, topk);
}

}  // namespace mi355
