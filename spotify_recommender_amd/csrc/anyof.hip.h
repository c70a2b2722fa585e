// anyof.hip.h — the ANY-OF scan (gfx950 only): the top-N rows by their BEST cosine among K <= 32 member queries q_0 .. q_{K-1}, and
// which member that was (engine_playlist.hip.h, include/mi355rec_diag.h "ANY-OF REQUESTS").
//
// Contract, per row x (bit for bit):
//     c_k(x) = cosine_with_norm(q_k, |q_k|, x, |x|)        (playlist.hip.h: core.hip.h's chain, the row's norm taken once;
//                                                           never NaN, in [-1, 1])
//     v(x) = c_0;  a(x) = 0;   for k = 1 .. K-1:  if (c_k > v) { v = c_k; a = k; }        (IEEE compare: -0.0 does not beat +0.0)
// Keys are pack_key(v, global row): ranked by v descending, then row ascending.  a(x) is the smallest member index that attains
// the maximum.  The compare chain selects one of the c_k: it adds no rounding, which is all the pre-filter's proof needs.
//
// OWN KERNEL, playlist_scan_kernel's launch: PlaylistCfg (512 threads, two workgroups per CU), tiles of 2048 rows dealt round-robin,
// the next tile's replica load in flight, PlaylistBuf as the call's inputs (weights, scales: never read).  playlist_scan_kernel sits
// at 128 VGPRs without scratch; a K-member loop inside its tile loop would have to be shown free for every other kind of request.
// What is shared is called, not copied: label_selected, filter_pass, rowset_admits, playlist_excluded, playlist_tile_quad,
// cosine_with_norm, compact_candidates, block_select_threshold, block_rank_and_store, the per-workgroup lists and merge.hip.h's
// merge; and the tile loop's pieces of playlist.hip.h ("THE SCAN'S SHARED PIECES"): scan_compact_at, scan_append (the ballot
// append), scan_exchange (the two barriers, the compaction and the shared_thr exchange), scan_quad_filter, scan_anchor_threshold
// (the anchor bound once the table is ranked: the pick, the rows read from the matrix and keyed by this file's anyof_row_key, the
// threshold) and scan_finish (the kernel's tail).  One piece is written out here as it is in playlist_scan_tiles, in the same
// order: the quad's admissible mask (tail mask, row-set nibble, four-label test), which as a function moved both kernels of this
// file by 1 - 2 VGPRs.
//
// ADMISSIBILITY is the playlist request's and is tested in its order: the row set's nibble and the label first (no fp32 row is
// read), then the pre-filter, then the feature filter on the fp32 rows left, then the K chains, and the exclusion list (LDS, binary
// search) only for a key that beats the workgroup's threshold.  Keys are formed only for admissible rows, so the rule "the k-th best
// key among ANY k admissible rows bounds the answer" keeps every workgroup threshold and the shared atomicMax valid.
//
// PRE-FILTER: playlist_cut.hip.h, "ANY": per member the PLAIN cut with K = 1; a row is ruled out only if every member rules it out.
// The members' digits, |u_k|, margins and integer cuts live in LDS (wave-uniform reads, moved to scalar registers); the cuts are
// refreshed by the first K threads whenever the workgroup's threshold moves.
//
// STARTING THRESHOLD, as playlist_anchor_bound: the anchor table's copy is ranked by the fp32 any-of value (it only CHOOSES rows),
// the best kPlBoundRows are read from the matrix, keyed exactly, the inadmissible ones dropped, and the topk-th best of the rest
// starts the threshold (0 where fewer remain, or topk > kPlBoundRows).
//
// ATTRIBUTION (AnyofArg::n_attr > 0, uniform): the same kernel, launched once more over the merged result: thread i reads key i of
// `attr_keys`, runs the K chains on that row and stores a(x) to attr_member[i] (-1 for an empty slot).  No second __global__.
//
// MANHATTAN (manhattan_scan_kernel, at the end of this file; include/mi355rec_diag.h "MANHATTAN REQUESTS"): a second kernel made of
// the same pieces.  It ranks by
//     d1_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fabsf(t))       (acc starts at 0.0f)
//     m(x)    = fl( fl(...fl(d1_0 + d1_1) + ... + d1_{K-1}) / (float)K ),     keys pack_key(-m, global row); m not finite: no key
// ascending in m, then row ascending.  Every piece below is a template on kL1: anyof_scan_kernel instantiates <false> and is the
// code it was, manhattan_scan_kernel instantiates <true>; the two share source, not a function.  What differs, in three places:
// the row key (anyof_row_key: manhattan_value in place of anyof_value), the anchor bound's ranking of the table (the same value; a
// value that is not finite is no candidate) and the cut (playlist_cut.hip.h, "MANHATTAN": the row's bytes times its stored norm,
// the PER-MEMBER L1 sum, a float compare; its three constants in LDS, kt refreshed by thread 0 whenever the threshold moves).
// `norms`: the handle's per-row norms (DISTANCE's), a quad's four loaded with the replica's tile, the next tile's in flight.
// Everything else (admissibility and its order, the candidate lists, the threshold exchange, rows_exact) is the source any-of
// runs.  The members' cosine constants (digits, |u_k|, margins) do not exist there.  DESIGN.md 5.4.18 has the registers and why
// the metric is not a branch of anyof_scan_kernel (it was, and any-of paid 1 % for it).
#pragma once

#include "playlist.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

struct AnyofArg {
    int k;            // members
    int n_excl;       // entries of PlaylistBuf::excl
    int by_row;       // 1: member m is the shard's row PlaylistBuf::rows[m]; 0: PlaylistBuf::members[m]
    uint32_t active;  // the feature filter (PlaylistArg::active)
    int labelled;     // 1: only rows whose label is in PlaylistBuf::label_mask are admissible
    const uint8_t* rowset;   // ROW SETS (PlaylistArg::rowset); null: no set
    uint32_t rowset_flip;
    int n_attr;       // > 0: ATTRIBUTION of attr_keys[0..n_attr), nothing is scanned
};

struct AnyofSmem {
    uint64_t* cand;
    SelectSmem& sel;
    int &count, &ok, &exact;
    unsigned long long& shared;
    float (*mem)[kDim];
    float* qn;
    uint32_t *excl, *lmask;
    int (*digits)[6];   // ANY: member k's query digits ...
    float *un, *margin; // ... |u_k| and margin_k ...
    int* cut;           // ... and its integer cut at the workgroup's threshold
    float* l1;          // MANHATTAN: ce, ke1 and kt of the cut (playlist_cut.hip.h)
};

struct AnyofCtx {
    const float *feats, *anchors;
    int64_t n, row_base;
    const PlaylistBuf* buf;
    unsigned long long* shared_thr;
    int k, n_excl, topk;
    uint32_t active;
    bool labelled;
    const int16_t* row_label;
    const uint2* labels4;
    const uint4* q8;
    const uint8_t* rowset;
    uint32_t flip;
    int tid, lane;
    const float4* norms4;  // MANHATTAN: a quad's four stored norms; null: none were passed (the cut is off)
};

// MANHATTAN: m(x) of the contract: the row's features once, K chains against the members in LDS, in order.
__device__ __forceinline__ float manhattan_value(const float (*__restrict__ mem)[kDim], int k, const Row& r) {
    float f[kDim];
    row_features(r, f);
    float sum = 0.0f;
    for (int m = 0; m < k; ++m) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < kDim; ++j) {
            const float t = mem[m][j] - f[j];
            acc = acc + __builtin_fabsf(t);
        }
        sum = m == 0 ? acc : sum + acc;
    }
    return sum / static_cast<float>(k);
}

// ... as a key on global row g: -m, or 0 where m is not finite (no key).
__device__ __forceinline__ uint64_t manhattan_key(const float (*__restrict__ mem)[kDim], int k, const Row& r, uint32_t g) {
    const float d = manhattan_value(mem, k, r);
    return d < __builtin_inff() ? pack_key(-d, g) : 0ull;   // (false for NaN)
}

// v(x) and a(x) of the contract: the row's features and norm once, K chains against the members in LDS, the compare chain.
__device__ __forceinline__ float anyof_value(const float (*__restrict__ mem)[kDim], const float* __restrict__ qn, int k, const Row& r, int& a) {
    float f[kDim];
    row_features(r, f);
    const float rn = query_norm(f);   // (the chain's own sum: sequential from 0.0f)
    float v = cosine_with_norm(mem[0], qn[0], f, rn);
    a = 0;
    for (int m = 1; m < k; ++m) {
        const float c = cosine_with_norm(mem[m], qn[m], f, rn);
        if (c > v) v = c, a = m;
    }
    return v;
}

// THE key of the fp32 row x at local row `row`: the anchor bound and the scan both call it (bit-identical keys).
template <bool kL1>
__device__ __forceinline__ uint64_t anyof_row_key(const AnyofCtx& c, const AnyofSmem& sm, const Row& x, int64_t row) {
    if constexpr (kL1) return manhattan_key(sm.mem, c.k, x, static_cast<uint32_t>(c.row_base + row));
    int a;
    return pack_key(anyof_value(sm.mem, sm.qn, c.k, x, a), static_cast<uint32_t>(c.row_base + row));
}

// ---- members and excluded ids into LDS; the members' norms; per member the ANY cut's constants.  Returns whether the cut is on.
template <bool kL1>
__device__ __forceinline__ bool anyof_prologue(const AnyofCtx& c, const AnyofSmem& sm, bool by_row) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    const PlaylistBuf* const buf = c.buf;
    const int tid = c.tid, k = c.k;
    for (int i = tid; i < k * kDim; i += kBlock)
        sm.mem[i / kDim][i % kDim] = by_row ? c.feats[buf->rows[i / kDim] * kDim + i % kDim] : buf->members[i / kDim][i % kDim];
    for (int i = tid; i < c.n_excl; i += kBlock) sm.excl[i] = buf->excl[i];
    if (c.labelled && tid < kMaxLabels / 32) sm.lmask[tid] = buf->label_mask[tid];
    if (tid == 0) sm.count = sm.exact = 0, sm.ok = 1;
    __syncthreads();
    if constexpr (kL1) {   // MANHATTAN: the cut's constants; it is off where a member's norm is not finite or above kBqMaxNorm
        if (tid < k) {
            float q[kDim];
#pragma unroll
            for (int j = 0; j < kDim; ++j) q[j] = sm.mem[tid][j];
            if (!(query_norm(q) <= kBqMaxNorm)) sm.ok = 0;   // (false for NaN; every writer writes 0)
        }
        if (tid == 0) {
            sm.l1[0] = 1.0f - playlist_cut_l1_eps(k);
            sm.l1[1] = static_cast<float>(k) * kL1HalfSteps;
            sm.l1[2] = __builtin_inff();   // no threshold yet: no row is ruled out
        }
        __syncthreads();
        return c.q8 != nullptr && c.norms4 != nullptr && sm.ok != 0;
    }
    if (tid < k) {
        float q[kDim];
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = sm.mem[tid][j];
        const float qn = query_norm(q);
        sm.qn[tid] = qn;
        int digits[6];
        float un, margin;
        // (a norm outside the range, NaN included: q / qn may be anything; the verdict below is then false)
        const bool in_range = qn >= kBqMinNorm && qn <= kBqMaxNorm;
        const bool on = playlist_cut_any_member(c.q8 != nullptr && in_range, q, qn, digits, un, margin);
#pragma unroll
        for (int j = 0; j < 6; ++j) sm.digits[tid][j] = digits[j];
        sm.un[tid] = un;
        sm.margin[tid] = margin;
        sm.cut[tid] = kPlCutNone;
        if (!on) sm.ok = 0;   // (every writer writes 0)
    }
    __syncthreads();
    return c.q8 != nullptr && sm.ok != 0;
}

// ---- the starting threshold (STARTING THRESHOLD above).  Returns the threshold key (published too), or 0.
template <bool kL1>
__device__ __forceinline__ uint64_t anyof_anchor_bound(const AnyofCtx& c, const AnyofSmem& sm, int& n_exact) {
    constexpr int kBlock = PlaylistCfg::kBlock, kPer = kAnchorRows / kBlock;
    const int tid = c.tid;
    const int64_t n = c.n;
    const int n_anchor = n < kAnchorRows ? static_cast<int>(n) : kAnchorRows;   // (anchor i is row i below kAnchorRows rows)
    if (!(c.anchors && c.topk <= kPlBoundRows && n_anchor >= kPlBoundRows)) return 0ull;   // uniform
    uint64_t mine[kPer];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int i = r * kBlock + tid;
        const Row a = load_row(c.anchors, static_cast<int64_t>(i));
        int who;
        if constexpr (kL1) mine[r] = i < n_anchor ? manhattan_key(sm.mem, c.k, a, static_cast<uint32_t>(i)) : 0ull;   // (not finite: no candidate)
        else mine[r] = i < n_anchor ? pack_key(anyof_value(sm.mem, sm.qn, c.k, a, who), static_cast<uint32_t>(i)) : 0ull;
        if (c.active && !filter_pass(a, c.active, c.buf->lo, c.buf->hi)) mine[r] = 0ull;   // (only chooses: re-checked on the matrix's row)
        if (c.labelled && i < n_anchor && !label_selected(sm.lmask, c.row_label[anchor_row(n, i)])) mine[r] = 0ull;
    }
    return scan_anchor_threshold(c, sm, mine, c.active || c.labelled || kL1,
                                 [&](const Row& x, int64_t row) { return anyof_row_key<kL1>(c, sm, x, row); }, n_exact);
}

// The workgroup's threshold key has moved: every member's cut, by the first K threads (the caller's barrier follows).
template <bool kL1>
__device__ __forceinline__ void anyof_cut_refresh(const AnyofCtx& c, const AnyofSmem& sm, uint64_t thr) {
    if constexpr (kL1) {   // MANHATTAN: kt = fl(K T), T = 0.0f - the threshold's score
        if (c.tid == 0) sm.l1[2] = static_cast<float>(c.k) * (0.0f - ordered_to_score(static_cast<uint32_t>(thr >> 32)));
    } else if (c.tid < c.k) sm.cut[c.tid] = playlist_cut_any(sm.un[c.tid], sm.margin[c.tid], ordered_to_score(static_cast<uint32_t>(thr >> 32)));
}

// ---- the scan: this workgroup's tiles, candidates into sm.cand (thr: the starting threshold key, or 0)
template <bool kL1>
__device__ __forceinline__ void anyof_scan_tiles(const AnyofCtx& c, const AnyofSmem& sm, bool cut_on, uint64_t thr, int& n_exact) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    const int tid = c.tid, lane = c.lane;
    const int64_t n = c.n, n_quads = (n + 3) >> 2, tiles = (n_quads + kBlock - 1) / kBlock;
    const int compact_at = scan_compact_at(c.topk);
    if (cut_on && thr != 0ull) {   // uniform
        anyof_cut_refresh<kL1>(c, sm, thr);
        __syncthreads();
    }
    HalfTile cur = {};
    uint2 cur_labels = make_uint2(0u, 0u);
    if (cut_on) cur = reinterpret_cast<const HalfTile*>(c.q8)[playlist_tile_quad(blockIdx.x, tid, n_quads)];
    if (c.labelled) cur_labels = c.labels4[playlist_tile_quad(blockIdx.x, tid, n_quads)];
    float4 cur_norms = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (kL1 && cut_on) cur_norms = c.norms4[playlist_tile_quad(blockIdx.x, tid, n_quads)];

    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform
        HalfTile nxt = cur;
        uint2 nxt_labels = cur_labels;
        // the next tile is in flight while this one is scored (past the last tile: the clamped quad again)
        if (cut_on) nxt = reinterpret_cast<const HalfTile*>(c.q8)[playlist_tile_quad(t + gridDim.x, tid, n_quads)];
        if (c.labelled) nxt_labels = c.labels4[playlist_tile_quad(t + gridDim.x, tid, n_quads)];
        float4 nxt_norms = cur_norms;
        if (kL1 && cut_on) nxt_norms = c.norms4[playlist_tile_quad(t + gridDim.x, tid, n_quads)];
        // (the quad's admissible mask stays written out here and in playlist_scan_tiles: as a function it moved anyof.hip.h's two kernels by 1 - 2 VGPRs)
        const int64_t quad = t * kBlock + tid;
        const int64_t r0 = quad * 4;
        const int64_t left = quad < n_quads ? n - r0 : 0;   // rows of the quad inside the shard
        uint32_t mask = left >= 4 ? 0xfu : (1u << static_cast<int>(left)) - 1u;
        if (c.rowset) {   // (uniform) ROW SETS: the quad's nibble, before anything else is done with its rows
            const int64_t q = playlist_tile_quad(t, tid, n_quads);
            mask &= ((static_cast<uint32_t>(c.rowset[q >> 1]) >> ((static_cast<uint32_t>(q) & 1u) * 4u)) ^ c.flip) & 0xfu;
        }
        if (c.labelled) {   // (uniform) the label test: it needs nothing but the label
            const int l4[4] = {static_cast<int16_t>(cur_labels.x & 0xffffu), static_cast<int16_t>(cur_labels.x >> 16),
                               static_cast<int16_t>(cur_labels.y & 0xffffu), static_cast<int16_t>(cur_labels.y >> 16)};
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4)
                if (!label_selected(sm.lmask, l4[u4])) mask &= ~(1u << u4);
        }
        if (cut_on && thr != 0ull) {   // (uniform) no threshold: every row is kept
            if constexpr (kL1) playlist_cut_l1_apply(mask, cur, cur_norms, sm.mem, c.k, sm.l1[0], sm.l1[1], sm.l1[2]);
            else playlist_cut_any_apply(mask, cur, sm.digits, sm.cut, c.k);
        }
        scan_quad_filter(c, r0, false, mask, n_exact);
        while (__ballot(mask != 0u)) {   // uniform
            const bool have = mask != 0u;
            const int64_t r = have ? r0 + __builtin_ctz(mask) : 0;
            const uint64_t row_key = anyof_row_key<kL1>(c, sm, load_row(c.feats, r), r);
            n_exact += (have && !c.active) ? 1 : 0;   // (with a filter every row read was counted above)
            const uint64_t key = have ? row_key : 0ull;
            bool pass = key > thr;
            if (pass && c.n_excl > 0) pass = !playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + r));
            scan_append(sm, lane, pass, key);
            mask &= mask - 1u;
        }
        const uint64_t before = thr;
        thr = scan_exchange(c, sm, compact_at, thr);
        if (cut_on && thr != before) {   // (uniform) every wave has left this tile's cut test: the barriers above
            anyof_cut_refresh<kL1>(c, sm, thr);
            __syncthreads();
        }
        cur = nxt;
        cur_labels = nxt_labels;
        cur_norms = nxt_norms;
    }
}

// ---- one workgroup's scan behind the prologue: the starting threshold, its tiles, the rows_exact count, the ranked list
template <bool kL1>
__device__ __forceinline__ void anyof_scan_body(const AnyofCtx& c, const AnyofSmem& sm, bool cut_on, uint64_t* __restrict__ block_lists,
                                                unsigned long long* __restrict__ rows_exact) {
    int n_exact = 0;   // rows whose K chains this thread computed
    uint64_t thr = 0ull;
    if (cut_on) thr = anyof_anchor_bound<kL1>(c, sm, n_exact);   // uniform
    anyof_scan_tiles<kL1>(c, sm, cut_on, thr, n_exact);
    scan_finish(c, sm, n_exact, block_lists, rows_exact);
}

// q8: the handle's 8-bit replica, or null (every row exact).  anchors: the anchor table, or null (no starting threshold).
// rows_exact: += the rows whose K chains the scan computed; with a filter, every fp32 row read (the attribution counts nothing).
// labels: the shard's labels in row order, four int16 to a quad (read only where arg.labelled).
// attr_keys, attr_member: ATTRIBUTION (arg.n_attr > 0): the merged keys, and where a(x) of each goes.
__global__ __launch_bounds__(PlaylistCfg::kBlock, PlaylistCfg::kMinWaves) void anyof_scan_kernel(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int64_t row_base, const PlaylistBuf* __restrict__ buf,
    AnyofArg arg, const float* __restrict__ anchors, int topk, uint64_t* __restrict__ block_lists,
    unsigned long long* __restrict__ rows_exact, unsigned long long* __restrict__ shared_thr /* &buf->shared_thr */,
    const uint2* __restrict__ labels, const uint64_t* __restrict__ attr_keys, int32_t* __restrict__ attr_member) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    __shared__ uint64_t s_cand[PlaylistCfg::kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count, s_ok, s_exact;
    __shared__ unsigned long long s_shared;
    __shared__ float s_mem[kMaxPlaylist][kDim];
    __shared__ float s_qn[kMaxPlaylist], s_un[kMaxPlaylist], s_margin[kMaxPlaylist];
    __shared__ int s_digits[kMaxPlaylist][6], s_cut[kMaxPlaylist];
    __shared__ uint32_t s_excl[kPlExcludeCap], s_lmask[kMaxLabels / 32];
    const AnyofSmem sm = {s_cand, s_sel, s_count, s_ok, s_exact, s_shared, s_mem, s_qn, s_excl, s_lmask, s_digits, s_un, s_margin, s_cut, nullptr};
    const int tid = threadIdx.x;
    const bool attribution = arg.n_attr > 0;   // uniform
    const AnyofCtx c = {feats, anchors, n, row_base, buf, shared_thr, arg.k, attribution ? 0 : arg.n_excl, topk, arg.active, arg.labelled != 0,
                        reinterpret_cast<const int16_t*>(labels), labels, attribution ? nullptr : q8, arg.rowset, arg.rowset_flip, tid, tid & 63,
                        nullptr};
    const bool cut_on = anyof_prologue<false>(c, sm, arg.by_row != 0);
    if (attribution) {   // (uniform) one thread per result: the K chains of its row, a(x) stored
        const int i = static_cast<int>(blockIdx.x) * kBlock + tid;
        if (i < arg.n_attr) {
            const uint64_t key = attr_keys[i];
            int a = -1;   // (an empty slot of the merged list)
            if (key != 0ull) {
                const int64_t row = static_cast<int64_t>(~static_cast<uint32_t>(key)) - row_base;
                (void)anyof_value(sm.mem, sm.qn, c.k, load_row(feats, row), a);
            }
            attr_member[i] = a;
        }
        return;
    }
    anyof_scan_body<false>(c, sm, cut_on, block_lists, rows_exact);
}

// MANHATTAN: the same pieces as their kL1 = true instances, in a kernel of its own (anyof_scan_kernel shares no function, no
// register allocation and no code layout with it).  The arguments are anyof_scan_kernel's without the attribution's; arg.n_attr is 0.
// norms: the rows' norms in row order, four fp32 to a quad, or null (no pre-filter then).
__global__ __launch_bounds__(PlaylistCfg::kBlock, PlaylistCfg::kMinWaves) void manhattan_scan_kernel(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int64_t row_base, const PlaylistBuf* __restrict__ buf,
    AnyofArg arg, const float* __restrict__ anchors, int topk, uint64_t* __restrict__ block_lists,
    unsigned long long* __restrict__ rows_exact, unsigned long long* __restrict__ shared_thr /* &buf->shared_thr */,
    const uint2* __restrict__ labels, const float4* __restrict__ norms) {
    __shared__ uint64_t s_cand[PlaylistCfg::kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count, s_ok, s_exact;
    __shared__ unsigned long long s_shared;
    __shared__ float s_mem[kMaxPlaylist][kDim];
    __shared__ float s_l1[4];
    __shared__ uint32_t s_excl[kPlExcludeCap], s_lmask[kMaxLabels / 32];
    // (the members' cosine constants are any-of's: never touched by a kL1 instance)
    const AnyofSmem sm = {s_cand, s_sel, s_count, s_ok, s_exact, s_shared, s_mem, nullptr, s_excl, s_lmask, nullptr, nullptr, nullptr, nullptr, s_l1};
    const int tid = threadIdx.x;
    const AnyofCtx c = {feats, anchors, n, row_base, buf, shared_thr, arg.k, arg.n_excl, topk, arg.active, arg.labelled != 0,
                        reinterpret_cast<const int16_t*>(labels), labels, q8, arg.rowset, arg.rowset_flip, tid, tid & 63, norms};
    const bool cut_on = anyof_prologue<true>(c, sm, arg.by_row != 0);
    anyof_scan_body<true>(c, sm, cut_on, block_lists, rows_exact);
}

}  // namespace mi355
