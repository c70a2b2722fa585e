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
// What is shared is included, not copied: label_selected, filter_pass, rowset_admits and the quad's nibble, playlist_excluded,
// playlist_tile_quad, cosine_with_norm, compact_candidates, block_select_threshold, block_rank_and_store, the per-workgroup lists
// and merge.hip.h's merge.  What a loop body is in playlist.hip.h and not a function (the ballot append, the two barriers and the
// shared_thr exchange, the anchor bound's pick-and-score) is written out again here, in the same order.
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
    static_assert(PlaylistCfg::kCandCap >= kAnchorRows / 2 && PlaylistCfg::kCandCap * 2 >= kPlBoundRows, "LDS reuse below");
    const int tid = c.tid, lane = c.lane;
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
    int n_cand = kPlBoundRows;   // anchors left to choose from: all of them without a filter
    if (c.active || c.labelled || kL1) {   // uniform
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const uint64_t have = __ballot(mine[r] != 0ull);
            if (lane == 0 && have) atomicAdd(&sm.count, __popcll(have));
        }
        __syncthreads();
        n_cand = sm.count;
        __syncthreads();
        if (tid == 0) sm.count = 0;
        __syncthreads();
    }
    // (fewer than kPlBoundRows candidates: keep them all)
    const uint64_t t = n_cand >= kPlBoundRows ? block_select_threshold<kBlock, kPer>(mine, kPlBoundRows, true, 0, sm.sel) : 1ull;
    int* const s_pick = reinterpret_cast<int*>(sm.cand);
#pragma unroll
    for (int r = 0; r < kPer; ++r) {   // (uniform loop) exactly kPlBoundRows keys are >= t, or all n_cand < kPlBoundRows
        const bool keep = mine[r] != 0ull && mine[r] >= t;
        const uint64_t who = __ballot(keep);
        int base = 0;
        if (lane == 0 && who) base = atomicAdd(&sm.count, __popcll(who));
        base = __builtin_amdgcn_readfirstlane(base);
        if (keep) s_pick[base + lanes_below(who)] = r * kBlock + tid;
    }
    __syncthreads();
    const int picked = sm.count;   // (<= kPlBoundRows <= kBlock)
    uint64_t key = 0ull;
    if (tid < picked) {
        const int64_t row = anchor_row(n, s_pick[tid]);
        const Row x = load_row(c.feats, row);   // from the matrix
        const bool x_pass = !c.active || filter_pass(x, c.active, c.buf->lo, c.buf->hi);
        const uint64_t row_key = anyof_row_key<kL1>(c, sm, x, row);
        ++n_exact;
        key = playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + row)) || !x_pass ||
                      (c.labelled && !label_selected(sm.lmask, c.row_label[row])) || (c.rowset && !rowset_admits(c.rowset, c.flip, row))
                  ? 0ull
                  : row_key;
    }
    const uint64_t have = __ballot(key != 0ull);
    __syncthreads();   // (every thread has read the count and s_pick)
    if (tid == 0) sm.count = 0;
    __syncthreads();
    if (lane == 0 && have) atomicAdd(&sm.count, __popcll(have));
    __syncthreads();
    const int usable = sm.count;
    __syncthreads();
    if (tid == 0) sm.count = 0;
    uint64_t thr = 0ull;
    if (usable >= c.topk) {   // uniform
        const uint64_t one[1] = {key};
        thr = block_select_threshold<kBlock, 1>(one, c.topk, true, 0, sm.sel) - 1ull;   // keys >= the topk-th pass
        if (tid == 0) atomicMax(c.shared_thr, static_cast<unsigned long long>(thr));
    }
    __syncthreads();
    return thr;
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
    int compact_at = 2 * c.topk > 256 ? 2 * c.topk : 256;
    if (compact_at > kCandLimit) compact_at = kCandLimit;
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
        if (c.active && mask != 0u) {   // (active uniform) the filter on the fp32 rows left, before any chain
            Row x[4];
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) x[u4] = load_row(c.feats, r0 + u4 < n ? r0 + u4 : n - 1);
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4)
                if (mask & (1u << u4)) {
                    ++n_exact;
                    if (!filter_pass(x[u4], c.active, c.buf->lo, c.buf->hi)) mask &= ~(1u << u4);
                }
        }
        while (__ballot(mask != 0u)) {   // uniform
            const bool have = mask != 0u;
            const int64_t r = have ? r0 + __builtin_ctz(mask) : 0;
            const uint64_t row_key = anyof_row_key<kL1>(c, sm, load_row(c.feats, r), r);
            n_exact += (have && !c.active) ? 1 : 0;   // (with a filter every row read was counted above)
            const uint64_t key = have ? row_key : 0ull;
            bool pass = key > thr;
            if (pass && c.n_excl > 0) pass = !playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + r));
            const uint64_t ballot = __ballot(pass);
            if (ballot) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&sm.count, __popcll(ballot));
                base = __builtin_amdgcn_readfirstlane(base);
                if (pass) sm.cand[base + lanes_below(ballot)] = key;
            }
            mask &= mask - 1u;
        }
        // two barriers: every wave reads the count before any wave appends again (scan_kernel)
        __syncthreads();
        const int count = sm.count;
        if (tid == 0) sm.shared = __hip_atomic_load(c.shared_thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint64_t published = sm.shared;
        const uint64_t before = thr;
        if (count >= compact_at) {
            const uint64_t local_thr = compact_candidates<kBlock, PlaylistCfg::kCandPerThread>(sm.cand, &sm.count, c.topk, false, sm.sel);
            if (local_thr > thr && local_thr > published && tid == 0) atomicMax(c.shared_thr, static_cast<unsigned long long>(local_thr));
            if (local_thr > thr) thr = local_thr;
        }
        if (published > thr) thr = published;
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
    constexpr int kBlock = PlaylistCfg::kBlock;
    int n_exact = 0;   // rows whose K chains this thread computed
    uint64_t thr = 0ull;
    if (cut_on) thr = anyof_anchor_bound<kL1>(c, sm, n_exact);   // uniform
    anyof_scan_tiles<kL1>(c, sm, cut_on, thr, n_exact);

    const int wave_exact = wave_inclusive_scan(n_exact);
    if (c.lane == 63 && wave_exact) atomicAdd(&sm.exact, wave_exact);
    __syncthreads();
    if (c.tid == 0 && rows_exact && sm.exact) atomicAdd(rows_exact, static_cast<unsigned long long>(sm.exact));
    if (sm.count > kRankCountMax && sm.count > c.topk)   // uniform
        compact_candidates<kBlock, PlaylistCfg::kCandPerThread>(sm.cand, &sm.count, c.topk, false, sm.sel);
    __syncthreads();
    block_rank_and_store<kBlock>(sm.cand, sm.count, block_lists + static_cast<int64_t>(blockIdx.x) * c.topk, c.topk);
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
