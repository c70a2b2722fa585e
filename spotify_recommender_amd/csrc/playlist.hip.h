// playlist.hip.h — the PLAYLIST scan (gfx950 only): the top-N rows by the WEIGHTED MEAN of their scores against K <= 32
// member queries q_0 .. q_{K-1} with signed weights w_0 .. w_{K-1}, a set of excluded rows left out (engine_playlist.hip.h,
// include/mi355rec_diag.h "PLAYLISTS" and "WEIGHTED PLAYLISTS").
//
// Contract, per row x (bit for bit):
//     c_k(x)   = cosine_score(q_k, |q_k|, x)                           (core.hip.h: the reference's chain)
//     W        = fl(...fl(|w_0| + |w_1|) + ... + |w_{K-1}|)            (fp32, member order; the host's sum, PlaylistArg::wsum)
//     score(x) = fl( fl(...fl( fl(w_0 c_0) + fl(w_1 c_1) ) + ... + fl(w_{K-1} c_{K-1}) ) / W )
// fp32, member order, multiply THEN add (never fused: fp contract is off below), one IEEE divide.  Keys are packed with the
// global row (ties break as in every other route), the excluded rows never listed.  An unweighted call is the call with
// every weight 1.0f: fl(1 c) = c and W = K exactly, so it is the plain mean fl(fl(c_0 + ... + c_{K-1}) / K) bit for bit and
// there is ONE code path.  Scores may be negative (dislikes): a key of any score is non-zero, thresholds are KEYS and 0
// means "no threshold yet", so nothing below assumes score >= 0.
//
// PRE-FILTER (playlist_cut.hip.h).  The weighted mean of the LINEAR cosines is one dot product u . x^, so one pass over the 8-bit
// replica (replica_q8.hip.h) bounds the ranking value of a row, and a row is ruled out iff its integer dot product D lies below
// a cut derived from the workgroup's threshold.  Which query the replica is asked, the cut of every kind of request (plain,
// prior, distance, scaled), when it is off for a launch, and the proof of each are in playlist_cut.hip.h; rows whose first byte is
// 0x80 (the replica's special rows) always take the K chains.  This file holds what a key CARRIES, which the cut never changes.
//
// STARTING THRESHOLD.  The rule: the k-th best key among ANY k or more distinct, not excluded rows bounds the k-th best key
// of the answer from below, so a workgroup may start from it.  Every workgroup ranks the handle's 4096-row anchor table
// (handoff.hip.h) by u, reads the best kPlBoundRows of those rows FROM THE MATRIX (the table may be stale for a borrowed
// matrix: it only chooses rows), scores them with the K chains, drops the excluded ones (the LDS list below) and starts
// from the topk-th best of the rest (0 when fewer than topk remain, or topk > kPlBoundRows).  All workgroups read the same
// rows: they are L2-resident after the first.
// The same rule makes every workgroup's own threshold (the topk-th best key of the rows IT has kept) a bound for all of
// them: a workgroup that raises its threshold publishes it (atomicMax on PlaylistBuf::shared_thr, reset by the host's
// copy of the call's inputs) and every workgroup takes the published maximum once per tile.  Monotone and valid whenever
// it is read, so no ordering is needed; on a catalogue of clusters the workgroups that hold the members' cluster lend
// their threshold to all the others.
//
// FEATURE FILTER (include/mi355rec_diag.h, "FEATURE FILTERS").  PlaylistArg::active (bit j: feature j constrained) and
// PlaylistBuf::lo / hi: a row x is admissible iff lo[j] <= x[j] && x[j] <= hi[j] for every active j, on the fp32 row of the
// matrix (IEEE compares: a NaN feature fails).  The 8-bit replica only rules rows out by similarity, so the pre-filter,
// its margin and the bound above are unchanged; the predicate is applied where an fp32 row is read:
//   * anchors: the anchor table's copy only CHOOSES the rows (rows failing the filter there are not picked); the rows read
//     from the matrix that fail are dropped like excluded ones, so the starting threshold is the topk-th best key among
//     admissible rows;
//   * scan: a lane whose quad still holds rows (after the pre-filter, or every row on the exact path and for 0x80 rows)
//     requests the quad's four fp32 rows together, drops the held ones that fail, and only then runs the K chains on the
//     rest: a rejected row costs one load and a few compares.
// So keys are only ever formed for admissible rows, and the rule above (the k-th best among ANY k admissible, not excluded
// rows bounds the answer) keeps every workgroup's threshold and the shared atomicMax valid.  rows_exact then counts every
// row read from the fp32 matrix (rejected ones included).  active == 0 takes none of these branches (uniform tests).
//
// LABEL SET (include/mi355rec_diag.h, "PLAYLIST REQUESTS").  PlaylistArg::labelled (uniform), PlaylistBuf::label_mask (bit l:
// label l is selected) and `labels`, the shard's labels in row order as int16 (engine_labels.hip.h: four to a quad, the last
// quad padded with -1): a row is admissible only if its label is >= 0 and selected.  The test needs no fp32 row, so it comes
// FIRST: per tile a lane loads its quad's four labels as one 8-byte load (the quad clamped by playlist_tile_quad as the replica load's is, issued
// with the next tile's replica load) and clears the mask bit of every row that fails, before the 8-bit dot products, the
// filter's fp32 loads and any chain — on the exact path too.  A row rejected by its label never reads an fp32 row and
// rows_exact does not count it.  The pre-filter, its margin and the argument of tests/test_playlist_margin.py do not change:
// the replica still only rules rows out by similarity, of the rows the label test has left.
//   * anchors: anchors whose row (anchor_row(n, i)) is not selected are not chosen; the rows then read from the matrix are
//     checked again, as the filter does, so the starting threshold is the topk-th best key among admissible rows;
//   * scan: as above.
// So keys are only ever formed for admissible rows here as well, and the rule (the k-th best among ANY k admissible, not
// excluded rows bounds the answer) keeps every workgroup's threshold and the shared atomicMax valid.  labelled == 0 takes
// none of these branches (uniform tests) and never reads `labels`.
//
// ROW PRIORS (include/mi355rec_diag.h, "ROW PRIORS").  PlaylistArg::prior (uniform), PlaylistArg::prior_weight = beta and
// `priors`, one fp32 p(x) per row in local row order (|p| <= 1, |beta| <= 4: checked by the host; the array is padded to whole
// quads).  The ranking value of a row is
//     v(x) = fl( score(x) + fl(beta p(x)) )                              (fp32, multiply THEN add: fp contract is off)
// and every key, every workgroup threshold and shared_thr is a key of v.  The rule above (the k-th best among ANY k admissible
// rows bounds the answer) does not care what the ranking value is, so the thresholds stay valid.
//   * exact path, 0x80 rows, survivors of the pre-filter: the chain loop reloads the row's prior (4 B, an L2 hit: four priors
//     are not kept live across the loop) and forms v with exactly those two operations;
//   * anchors: the anchor table still only CHOOSES rows (by similarity alone); the rows read from the matrix get their prior
//     added before the starting threshold is taken, so that threshold is a key of v;
//   * pre-filter: per tile a lane loads its quad's four priors as one 16-byte load (the quad clamped as the replica load clamps
//     it, issued with the next tile's replica load): the per-row cut of playlist_cut.hip.h, "PRIOR".
// prior == 0 takes none of these branches (uniform tests) and never reads `priors`.
//
// DISTANCE (include/mi355rec_diag.h, "DISTANCE REQUESTS").  PlaylistArg::metric == kPlDistance (uniform): the ranking value of
// a row is the MEAN SQUARED EUCLIDEAN DISTANCE to the members, smaller is better:
//     d2_k(x) = acc after j = 0..11 of:  t = fl(q_kj - x_j);  acc = fl(acc + fl(t * t))        (acc starts at 0.0f)
//     m(x)    = fl( fl(...fl(d2_0 + d2_1) + ... + d2_{K-1}) / (float)K )                       (member order; K = 1: m = d2_0)
// fp32, subtract, multiply THEN add (fp contract is off), one IEEE divide (by 1.0f for K = 1: exact).  Every key, every
// workgroup threshold and shared_thr is a key of -m: pack_key orders by score descending, so the best keys are the nearest
// rows, ties break by global row ascending as everywhere, and m = +0.0 packs as a score of +0.0 (score_to_ordered maps -0.0
// there).  The rule above (the k-th best key among ANY k admissible rows bounds the answer) does not care what the ranking
// value is, so selection, compaction, the per-workgroup lists, the shared atomicMax and the merge are unchanged.  The host
// reports sqrtf(m) (engine_playlist.hip.h); the weights, W and the priors are never read.
//   * a row whose m is not finite (NaN or inf: hostile features or members, an overflowing sum) forms NO key: it is not
//     admissible, like a row the filter rejects;
//   * the K chains (playlist_sqdist) replace playlist_mean where a key is formed; exclusion lookup, filter and the label
//     test first are as above;
//   * PRE-FILTER: playlist_cut.hip.h, "DISTANCE" (the replica is queried with the centroid; a per-row cut from the row's norm).
//   * PER-ROW NORMS.  `norms`: s(x) = sqrtf of the sequential fp32 sum of squares, one fp32 per row in local row order, padded
//     to whole quads (q8_build_kernel's second output, launched with a null replica pointer by the handle's first distance
//     request; engine_playlist.hip.h says who owns it).  Per tile a lane loads its quad's four norms as one 16-byte load, with
//     the next tile's replica load, in the registers the priors' load uses (a distance request has no prior).
//   * STARTING THRESHOLD.  The rule above holds for any ranking value: the anchor table's copy is ranked by the chain's d2
//     against c (anchors whose d2 is not finite are not chosen), the best kPlBoundRows are read from the matrix and scored
//     with the K chains, and the topk-th best admissible one starts the threshold.
// metric == kPlCosine takes none of these branches (uniform tests).
//
// FEATURE SCALES (include/mi355rec_diag.h, "FEATURE SCALES").  PlaylistArg::scaled (uniform) and PlaylistBuf::scales = a_0 .. a_11
// (finite, 0 <= a_j <= 1024, not all zero: checked by the host; in LDS as s_scale).  The request is the unscaled request of
// either metric on rows x'_j = fl(a_j x_j) and members q'_kj = fl(a_j q_kj), one fp32 multiply each:
//   * members: scaled once in the prologue as they enter LDS (a member given by row after its row is read), so the members'
//     norms, u, the centroid and Q2 are those of the scaled members with no further change;
//   * exact chains (the exact path, 0x80 rows, survivors of the pre-filter, the anchor rows read from the matrix): the loaded
//     Row is scaled once (scale_row: 12 multiplies, not once per member), then playlist_mean / playlist_sqdist run unchanged;
//   * the feature filter tests the row BEFORE it is scaled (the stored x); labels and exclusion do not read features;
//   * anchors: the table's copy is scaled and ranked by u (by the chain's d2 for the distance metric).  It only chooses rows, and
//     the rule (the k-th best key among ANY k admissible rows bounds the answer) holds for any ranking value, so the shared
//     atomicMax, selection and merge are unchanged;
//   * DISTANCE with scales runs on the exact path: the host passes null `norms` (they are the unscaled rows' norms).
//   * PRE-FILTER, cosine metric: playlist_cut.hip.h, "SCALED" (the replica is queried with ubar = Abar u; a per-row cut from the
//     row's own replica bytes).
// scaled == 0 takes none of these branches (uniform tests) and never reads PlaylistBuf::scales.
//
// ROW SETS (include/mi355rec_diag.h, "ROW SETS").  PlaylistArg::rowset (uniform; null: no set), the shard's bitmap built on the host
// (rowset.h, engine_rowset.hip.h): bit i & 7 of byte i / 8 is local row i, the bits past the last row are 0; and PlaylistArg::rowset_flip:
// 0xf when rows IN the set are not admissible (EXCLUDE), 0 when rows NOT in it are not (ONLY), so (nibble ^ flip) & 0xf is a quad's
// admissible mask.  Like the label test it needs no fp32 row, so it comes FIRST:
//   * scan: per tile a lane takes the nibble of its quad (byte quad >> 1, shift (quad & 1) * 4, the quad clamped by playlist_tile_quad)
//     and ANDs it into `mask` before the label test, the 8-bit dot products, the filter's fp32 loads and any chain, on the exact path
//     and for the replica's 0x80 rows too.  A row the set rejects never reads an fp32 row and rows_exact does not count it.  The byte is
//     loaded at the top of the tile iteration, not with the next tile's replica load: measured both ways at 128 VGPRs and no scratch
//     (docs/LAB_NOTES.md): the prefetched form takes about 2 us off a K = 1 call with a set at 10 M rows and was not shown to leave
//     the calls without a set alone, which this form does;
//   * anchors: the rows read from the matrix are tested again, beside playlist_excluded, the filter and the label, so the starting
//     threshold stays the topk-th best key among admissible rows (the anchor table's copy still only chooses rows, by similarity).
// So keys are only ever formed for admissible rows, and the rule (the k-th best among ANY k admissible rows bounds the answer) keeps
// every workgroup's threshold and the shared atomicMax valid.  The pre-filter, its margins and playlist_cut.hip.h do not change: the
// replica still only rules rows out by similarity, among the rows the set has left.  rowset == null takes none of these branches
// (uniform tests) and reads nothing new.
//
// CANDIDATE LISTS (include/mi355rec_diag.h, "CANDIDATE LISTS").  PlaylistArg::cand (uniform; null: no list): this shard's listed
// rows, local, strictly ascending, as uint32 (candidates.h, engine_playlist.hip.h).  The kernel then GATHERS: playlist_gather_rows
// takes the place of playlist_anchor_bound + playlist_scan_tiles, the prologue before it and the tail after it are shared.  The
// host launches it with a null replica, null anchors and null norms: the cut is off, the threshold starts at 0 and every listed
// row takes the exact chain, so the keys are those of the exact path by construction (playlist_row_key).
//   * workgroup b takes the entries [(b + j gridDim.x) kBlock kPlGatherPerThread, + kBlock kPlGatherPerThread), j = 0, 1, ...; a
//     thread takes kPlGatherPerThread consecutive entries and requests their fp32 rows TOGETHER (one memory round trip after the
//     one for the entries, as the filter path requests a quad's four rows); an entry past n_cand re-reads the last one, masked;
//   * per entry, in the scan's order: the row-set bit, the label (by row: the list knows nothing of quads), the filter on the
//     stored row, then playlist_row_key, playlist_excluded and the ballot append.  rows_exact counts every entry that reaches the
//     filter or the chains;
//   * per iteration the scan's two barriers, compact_candidates at compact_at and the shared_thr exchange: an iteration appends at
//     most kBlock kPlGatherPerThread <= PlaylistCfg::kTileRows keys, a tile's worth, so the candidate slots cannot overflow.
// The rows ascend, so neighbouring lanes share cache lines where the list is dense.  cand == null takes none of this (one uniform
// test in the kernel body) and the scan's loop is untouched.
//
// CANDIDATE SCORES (include/mi355rec_diag.h, "CANDIDATE SCORES").  The gather launched with topk == 0 (uniform) and, as `block_lists`,
// a buffer of n_cand 64-bit words: the SCORE MODE.  For entry e of the list the thread stores word e: the row's playlist_row_key if
// the row passed the row-set, label and filter tests, formed a key and is not in the LDS exclusion list, else 0.  The threshold stays
// 0, so every formed key is looked up in the exclusion list.  Nothing is appended: the ballot, the two barriers, the compaction and
// the shared_thr exchange are skipped, sm.count stays 0, the tail stores topk = 0 keys per workgroup and the host launches no merge.
// Entries past n_cand store nothing.  No kernel argument is added (the kernel sits on its register budget): the mode rides on topk,
// the buffer on block_lists.
//
// BOUNDED (include/mi355rec_diag.h, "BOUNDED REQUESTS").  The scan (no candidate list) launched with topk == 0 (uniform): the
// COUNT MODE.  PlaylistBuf::shared_thr holds the request's FLOOR, a key threshold the host derived from its bound, and the launch
// counts the rows whose key exceeds it: the workgroup's threshold starts at the floor (the anchor bound is skipped: it needs a
// topk) and never moves, so the cut is the final one from the first tile.  A row the cut leaves takes the exact chains as in
// every other launch; key > thr, then the exclusion lookup, decides whether it MATCHES.  A match is counted where the other
// launches count a chain (n_exact) and is not appended: sm.count stays 0, nothing compacts, nothing is published (the two
// barriers and the shared_thr read remain: the word holds the floor and changes nothing).  The host passes a per-call total word
// as `rows_exact`; the tail stores topk = 0 keys per workgroup and no merge follows.  No kernel argument is added: the mode rides
// on topk as the gather's score mode does (with a candidate list topk == 0 is still that).  Filter, label set, row set, the
// special rows and the exact path (no replica, the cut off) are untouched, so the count is exact under all of them.
//   * PROVEN IN (playlist_cut.hip.h, "BOUNDED"): with the plain cut and no filter, a valid row whose D reaches cut_hi is proven to
//     match by the replica alone: it goes through the exclusion lookup and is counted, and its fp32 row is never read.  The rows
//     between the two cuts take the chains.  PlaylistArg::n_cand != 0 without a list turns the shortcut off (only the experiments
//     build's host ever passes that: the A/B of tools/run_bounded.py); the count is the same either way.
//
// JACCARD (include/mi355rec_diag.h, "JACCARD REQUESTS").  PlaylistArg::metric == kPlJaccard (uniform): the ranking value of a row is
// the MEAN WEIGHTED JACCARD (Ruzicka) SIMILARITY to the members, larger is better.  Everything fp32, in this order, never fused:
//     num = den = 0.0f
//     for j = 0..11:  lt = x_j < q_kj;  lo = lt ? x_j : q_kj;  hi = lt ? q_kj : x_j;  num = fl(num + lo);  den = fl(den + hi)
//     J_k  = fl(num / den)                                                           (one IEEE divide)
//     v(x) = fl( fl(...fl(J_0 + J_1) + ... + J_{K-1}) / (float)K )                   (member order; K = 1 divides by 1.0f: exact)
// min and max are ONE compare and two selects, not fminf / fmaxf (which drop a NaN): a NaN in the row reaches den (x_j < q_kj is
// false, hi = x_j) and a NaN in a member reaches num (lo = q_kj).  Keys are pack_key(v, global row): v descending, then row
// ascending, as the cosine request's.  A row forms a key only if v is finite AND every den_k is below +inf (a +inf feature would
// otherwise score a quiet 0: finite / inf): two all-zero vectors (0 / 0), NaN and infinite features are never returned.  The formula
// is applied as written whatever the signs; it is the Ruzicka similarity, in [0, 1], where row and members are non-negative.
//   * the K chains (playlist_jaccard) replace playlist_mean where a key is formed (playlist_row_key: the scan, the gather and the
//     anchor rows read from the matrix all carry the same bits); exclusion lookup, filter, label test and row set are as above;
//   * the weights (the prologue still copies the host's 1.0f each), W, u and the members' norms never enter a key; the priors are
//     never read and `norms` is never passed;
//   * NO PRE-FILTER: the host launches with a null replica, so the cut is off, the threshold starts at 0 and every admissible row
//     takes the chains (docs/LAB_NOTES.md has the forms of an 8-bit bound that were tried and their register figures).
// metric == kPlCosine takes none of these branches (uniform tests).
//
// EXCLUSION.  The excluded global ids (members and the caller's list, sorted and deduplicated on the host, at most
// kPlExcludeCap) sit in LDS as uint32; only a key that already beats the workgroup's threshold is looked up (binary
// search), so the hot loop does not change.
//
// Tiles of 2048 rows (one quad of four rows per lane, the replica's packing) are dealt round-robin over the workgroups;
// without a replica the same tiles are read from the fp32 rows, every row exact (a runtime branch, not a second
// instantiation).  Selection, compaction and the per-workgroup lists are label_scan_kernel's; the merge of merge.hip.h
// follows.
#pragma once

#include "labels.hip.h"
#include "playlist_cut.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kMaxPlaylist = 32;                            // MI355REC_MAX_PLAYLIST
constexpr int kMaxExclude = 1024;                           // MI355REC_MAX_EXCLUDE
constexpr int kPlExcludeCap = kMaxExclude + kMaxPlaylist;   // the caller's ids and the members' rows
constexpr int kPlBoundRows = 256;                           // anchor rows a workgroup scores for its starting threshold
constexpr int kPlCosine = 0, kPlDistance = 1, kPlJaccard = 2;   // PlaylistArg::metric
using PlaylistCfg = Q8Cfg<512, 4, 1>;                       // kBlock, kMinWaves (two workgroups per CU); tiles of 2048 rows

// One call's inputs on the device (written by the host before the launch).
struct PlaylistBuf {
    float members[kMaxPlaylist][kDim];
    int64_t rows[kMaxPlaylist];
    float lo[kDim];                  // the feature filter's bounds (read only where PlaylistArg::active has bit j)
    float hi[kDim];
    float weights[kMaxPlaylist];     // w_k, checked by the host (1.0f each for an unweighted call)
    float scales[kDim];              // FEATURE SCALES a_j, checked by the host (read only where PlaylistArg::scaled)
    unsigned long long shared_thr;   // the best threshold any workgroup of the launch has found (0 from the host)
    uint32_t label_mask[kMaxLabels / 32];   // the label set (read only where PlaylistArg::labelled): bit l = label l is selected
    uint32_t excl[kPlExcludeCap];   // sorted, distinct global ids (only those of this shard)
};

struct PlaylistArg {
    int k;            // members
    int n_excl;       // entries of PlaylistBuf::excl
    int by_row;       // 1: member m is the shard's row PlaylistBuf::rows[m]; 0: PlaylistBuf::members[m]
    uint32_t active;  // the feature filter: bit j (j < kDim) constrains feature j; 0: no filter
    float wsum;       // W = fl(sum_k |w_k|) in member order (the host's fp32 sum; K for an unweighted call)
    int labelled;     // 1: only rows whose label is in PlaylistBuf::label_mask are admissible; 0: no label set
    float prior_weight;   // beta (read only where `prior`): v = fl(score + fl(beta p(x)))
    int prior;        // 1: rank by v, p from the kernel's `priors`; 0: rank by the score alone (`priors` is never read)
    int metric;       // kPlCosine, or kPlDistance: rank by -m(x), the mean squared distance to the members (DISTANCE above), or
                      // kPlJaccard: rank by v(x), the mean weighted Jaccard similarity to the members (JACCARD above)
    int scaled;       // 1: rows and members are multiplied by PlaylistBuf::scales before the chains (FEATURE SCALES above); 0: never read
    const uint8_t* rowset;   // ROW SETS above: the shard's bitmap, bit i of byte i / 8 is local row i (padding bits 0); null: no set
    uint32_t rowset_flip;    // ... 0xf: rows IN the set are not admissible (EXCLUDE); 0: rows NOT in it are not (ONLY)
    const uint32_t* cand;    // CANDIDATE LISTS above: n_cand > 0 local rows, strictly ascending: only they are read; null: no list
    int64_t n_cand;
};

// Is label l (int16 of the row-order array: -1 = unlabelled or padding) in the set?
__device__ __forceinline__ bool label_selected(const uint32_t* s_lmask, int l) {
    return l >= 0 && ((s_lmask[(l & (kMaxLabels - 1)) >> 5] >> (l & 31)) & 1u) != 0u;
}

// The feature filter's predicate on one fp32 row (active: uniform; unrolled, so no feature is indexed at run time).
__device__ __forceinline__ bool filter_pass(const Row& r, uint32_t active, const float* __restrict__ lo, const float* __restrict__ hi) {
    float f[kDim];
    row_features(r, f);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kDim; ++j)
        if (active & (1u << j)) ok = ok && lo[j] <= f[j] && f[j] <= hi[j];   // (false for a NaN feature)
    return ok;
}

// FEATURE SCALES: x'_j = fl(a_j x_j), one multiply per feature (a: LDS).
__device__ __forceinline__ void scale_row(Row& r, const float* __restrict__ a) {
    r.a = make_float4(a[0] * r.a.x, a[1] * r.a.y, a[2] * r.a.z, a[3] * r.a.w);
    r.b = make_float4(a[4] * r.b.x, a[5] * r.b.y, a[6] * r.b.z, a[7] * r.b.w);
    r.c = make_float4(a[8] * r.c.x, a[9] * r.c.y, a[10] * r.c.z, a[11] * r.c.w);
}

// cosine_score with the row's features f and norm rn = sqrtf(sum f_j^2) taken once for all members: the same operations in the same order.
__device__ __forceinline__ float cosine_with_norm(const float* __restrict__ q, float qn, const float (&f)[kDim], float rn) {
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < kDim; ++j) dot = dot + q[j] * f[j];
    const float den = rn * qn;
    float s = 0.0f;
    if (den > 1e-8f) {
        const float t = dot / den;
        const float m = (t < 1.0f) ? t : 1.0f;
        s = (-1.0f < m) ? m : -1.0f;
    }
    return s;
}

// The contract's score of one row: members and weights (LDS) in order, multiply then add in fp32, one divide by W.
__device__ __forceinline__ float playlist_mean(const float (*__restrict__ mem)[kDim], const float* __restrict__ qn,
                                               const float* __restrict__ w, float wsum, int k, const Row& r) {
    float f[kDim];
    row_features(r, f);
    const float rn = query_norm(f);   // (the chain's own sum: sequential from 0.0f)
    float sum = w[0] * cosine_with_norm(mem[0], qn[0], f, rn);
    for (int m = 1; m < k; ++m) sum = sum + w[m] * cosine_with_norm(mem[m], qn[m], f, rn);
    return sum / wsum;
}

// DISTANCE: sum_j q_j^2, sequential fp32 (what query_norm takes the root of).
__device__ __forceinline__ float playlist_sqnorm(const float (&q)[kDim]) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kDim; ++j) s = s + q[j] * q[j];
    return s;
}

// DISTANCE: m(x), the contract's mean squared distance of one row to the members (LDS) in order.
__device__ __forceinline__ float playlist_sqdist(const float (*__restrict__ mem)[kDim], int k, const Row& r) {
    float f[kDim];
    row_features(r, f);
    float sum = 0.0f;
    for (int m = 0; m < k; ++m) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < kDim; ++j) {
            const float t = mem[m][j] - f[j];
            acc = acc + t * t;
        }
        sum = m == 0 ? acc : sum + acc;
    }
    return sum / static_cast<float>(k);
}

// JACCARD: v(x), the contract's mean weighted Jaccard similarity of one row to the members (LDS) in order; *bounded: every den_k < +inf.
__device__ __forceinline__ float playlist_jaccard(const float (*__restrict__ mem)[kDim], int k, const Row& r, bool* bounded) {
    float f[kDim];
    row_features(r, f);
    float sum = 0.0f;
    bool ok = true;
    for (int m = 0; m < k; ++m) {
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int j = 0; j < kDim; ++j) {
            const float q = mem[m][j];
            const bool lt = f[j] < q;   // (one compare, two selects: a NaN goes where the contract says)
            num = num + (lt ? f[j] : q);
            den = den + (lt ? q : f[j]);
        }
        ok = ok && den < __builtin_inff();   // (false for NaN)
        const float jk = num / den;
        sum = m == 0 ? jk : sum + jk;
    }
    *bounded = ok;
    return sum / static_cast<float>(k);
}

// ROW SETS: does the set admit local row `row`?  (bits: non-null)
__device__ __forceinline__ bool rowset_admits(const uint8_t* __restrict__ bits, uint32_t flip, int64_t row) {
    return (((static_cast<uint32_t>(bits[row >> 3]) >> (row & 7)) ^ flip) & 1u) != 0u;
}

__device__ __forceinline__ bool playlist_excluded(const uint32_t* s_excl, int n_excl, uint32_t g) {
    int lo = 0, hi = n_excl;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_excl[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_excl && s_excl[lo] == g;
}

// The workgroup's LDS as the pieces below see it.  The kernel declares every array on its own and binds it here: the compiler then
// knows that no two of them alias and lays them out itself (one struct IN LDS costs the kernel registers it does not have).
struct PlaylistSmem {
    uint64_t* cand;
    SelectSmem& sel;
    int &count, &ok, &exact;
    unsigned long long& shared;
    float (*mem)[kDim];
    float *qn, *w, *u;
    uint32_t *excl, *lmask;
    float *scale, *abar;   // FEATURE SCALES: a_j and a_j / a_max (both only where arg.scaled)
};

// What every piece of the kernel reads: its arguments, spelled out once (all uniform but tid and lane).
struct PlaylistCtx {
    const float *feats, *anchors;
    int64_t n, row_base;
    const PlaylistBuf* buf;
    unsigned long long* shared_thr;
    int k, n_excl, topk;
    uint32_t active;
    float wsum, beta;
    bool by_row, labelled, prior, dist, scaled, jaccard;
    const int16_t* row_label;   // the rows' labels one by one, and four to a quad
    const uint2* labels4;
    const float* row_prior;     // the rows' priors one by one
    const float4* side4;        // a quad's four SIDE values: the rows' priors, or (DISTANCE) their stored norms; null: none were passed
    const uint4* q8;            // (never read with the cut off)
    const uint8_t* rowset;      // ROW SETS: the bitmap, or null
    uint32_t flip;
    int tid, lane;
};

// THE value a key carries, written once: the key of the fp32 row x (as stored: scaled here) at local row `row`, or 0 where the
// ranking value is not finite (DISTANCE).  The anchor bound and the scan both call it: the starting threshold is only valid
// because they form bit-identical keys.  Filter, label set and exclusion are the caller's.
__device__ __forceinline__ uint64_t playlist_row_key(const PlaylistCtx& c, const PlaylistSmem& sm, Row x, int64_t row) {
    if (c.scaled) scale_row(x, sm.scale);   // (uniform) FEATURE SCALES: once per row, then the chains unchanged
    float m;
    bool finite = true;
    if (c.dist) {   // (uniform) DISTANCE: the key carries -m; a row whose m is not finite forms no key
        const float d = playlist_sqdist(sm.mem, c.k, x);
        finite = d < __builtin_inff();   // (false for NaN)
        m = -d;
    } else if (c.jaccard) {   // (uniform) JACCARD: the key carries v; not finite, or a den_k that is not below +inf, forms no key
        m = playlist_jaccard(sm.mem, c.k, x, &finite);
        finite = finite && __builtin_fabsf(m) < __builtin_inff();   // (false for NaN)
    } else {
        m = playlist_mean(sm.mem, sm.qn, sm.w, c.wsum, c.k, x);
    }
    if (c.prior) m = m + c.beta * c.row_prior[row];   // (uniform) v: multiply, round, add, round; the prior is an L2 hit in the scan
    return finite ? pack_key(m, static_cast<uint32_t>(c.row_base + row)) : 0ull;
}

// ---- members and excluded ids into LDS; the members' norms; u and its norm; the launch's cut and the replica's query
__device__ __forceinline__ Q8Query playlist_prologue(const PlaylistCtx& c, const PlaylistSmem& sm, float (&u)[kDim], float& un, PlaylistCut& cut) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    const PlaylistBuf* const buf = c.buf;
    const int tid = c.tid, k = c.k;
    float* const s_q2 = sm.w;   // DISTANCE: |q_k|^2 for Q2, in the weights' LDS
    for (int i = tid; i < k * kDim; i += kBlock) {
        const float q = c.by_row ? c.feats[buf->rows[i / kDim] * kDim + i % kDim] : buf->members[i / kDim][i % kDim];
        sm.mem[i / kDim][i % kDim] = c.scaled ? buf->scales[i % kDim] * q : q;   // (uniform) FEATURE SCALES: q'_kj = fl(a_j q_kj)
    }
    float a_max = 1.0f;
    if (c.scaled) {   // uniform
        a_max = buf->scales[0];
#pragma unroll
        for (int j = 1; j < kDim; ++j) a_max = __builtin_fmaxf(a_max, buf->scales[j]);
        if (tid < kDim) {
            sm.scale[tid] = buf->scales[tid];
            sm.abar[tid] = buf->scales[tid] / a_max;   // (the host has checked a_max > 0)
        }
    }
    for (int i = tid; i < c.n_excl; i += kBlock) sm.excl[i] = buf->excl[i];
    if (c.labelled && tid < kMaxLabels / 32) sm.lmask[tid] = buf->label_mask[tid];
    if (tid == 0) sm.count = sm.exact = 0, sm.ok = 1;
    __syncthreads();
    if (tid < k) {
        float q[kDim];
#pragma unroll
        for (int j = 0; j < kDim; ++j) q[j] = sm.mem[tid][j];
        const float qn = query_norm(q);
        sm.qn[tid] = qn;
        if (c.dist) s_q2[tid] = playlist_sqnorm(q);   // (uniform)
        else sm.w[tid] = buf->weights[tid];
        if (!(qn >= kBqMinNorm && qn <= kBqMaxNorm)) sm.ok = 0;   // (false for NaN too; every writer writes 0)
    }
    __syncthreads();
    if (tid < kDim) {   // u: the weighted mean of the members' unit vectors (only used where every |q_k| is in range)
        if (c.dist) {   // (uniform) DISTANCE: u is the centroid c = fl(fl(q_0j + ... + q_{K-1}j) / K)
            float sum = sm.mem[0][tid];
            for (int m = 1; m < k; ++m) sum = sum + sm.mem[m][tid];
            sm.u[tid] = sum / static_cast<float>(k);
        } else {
            float sum = sm.w[0] * (sm.mem[0][tid] / sm.qn[0]);
            for (int m = 1; m < k; ++m) sum = sum + sm.w[m] * (sm.mem[m][tid] / sm.qn[m]);
            sm.u[tid] = sum / c.wsum;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kDim; ++j) u[j] = sm.u[j];
    un = query_norm(u);
    return playlist_cut_setup(cut, c.q8 != nullptr && sm.ok != 0, c.side4 != nullptr, c.dist, c.scaled, c.prior, c.beta, k, u, un, a_max,
                              sm.abar, sm.qn, s_q2);
}

// ---- THE SCAN'S SHARED PIECES.  The family's three kernels (this file's, and anyof.hip.h's two) call them; Ctx / Smem are
// PlaylistCtx / PlaylistSmem or AnyofCtx / AnyofSmem, which name what these pieces touch alike.  The starting threshold and the
// shared atomicMax are valid only because every kernel applies the same rule in the same order: it is written here, once.

// The candidate count at which a workgroup compacts its list: 2 topk, at least 256, at most kCandLimit.
__device__ __forceinline__ int scan_compact_at(int topk) {
    const int at = 2 * topk > 256 ? 2 * topk : 256;
    return at > kCandLimit ? kCandLimit : at;
}

// The ballot append: the keys of the wave's passing lanes into sm.cand, one LDS atomic per wave.
template <class Smem>
__device__ __forceinline__ void scan_append(const Smem& sm, int lane, bool pass, uint64_t key) {
    const uint64_t ballot = __ballot(pass);
    if (ballot) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&sm.count, __popcll(ballot));
        base = __builtin_amdgcn_readfirstlane(base);
        if (pass) sm.cand[base + lanes_below(ballot)] = key;
    }
}

// The end of a tile: two barriers (every wave reads the count before any wave appends again: scan_kernel), the published
// threshold read once for the workgroup, the compaction at compact_at, and the exchange: a workgroup that raised its threshold
// above the published one publishes it, and every workgroup adopts the published maximum.  Returns the new threshold.
template <class Ctx, class Smem>
__device__ __forceinline__ uint64_t scan_exchange(const Ctx& c, const Smem& sm, int compact_at, uint64_t thr) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    __syncthreads();
    const int count = sm.count;
    if (c.tid == 0) sm.shared = __hip_atomic_load(c.shared_thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint64_t published = sm.shared;
    if (count >= compact_at) {
        const uint64_t local_thr = compact_candidates<kBlock, PlaylistCfg::kCandPerThread>(sm.cand, &sm.count, c.topk, false, sm.sel);
        if (local_thr > thr && local_thr > published && c.tid == 0) atomicMax(c.shared_thr, static_cast<unsigned long long>(local_thr));
        if (local_thr > thr) thr = local_thr;
    }
    return published > thr ? published : thr;
}

// The feature filter on the fp32 rows the quad at r0 still holds, before any chain.  The quad's four rows are requested together
// (one memory round trip, not four); rows past n read row n - 1.  counting (BOUNDED): n_exact counts matches, not the rows read.
template <class Ctx>
__device__ __forceinline__ void scan_quad_filter(const Ctx& c, int64_t r0, bool counting, uint32_t& mask, int& n_exact) {
    if (c.active && mask != 0u) {   // (active uniform)
        Row x[4];
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4) x[u4] = load_row(c.feats, r0 + u4 < c.n ? r0 + u4 : c.n - 1);
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4)
            if (mask & (1u << u4)) {
                n_exact += counting ? 0 : 1;
                if (!filter_pass(x[u4], c.active, c.buf->lo, c.buf->hi)) mask &= ~(1u << u4);
            }
    }
}

// The starting threshold once the anchor table is ranked (mine: a thread's keys of the table's copy, 0 for an anchor that is
// no candidate): the best kPlBoundRows are picked, read FROM THE MATRIX, keyed by row_key(x, row) (the scan's own key of the
// kernel), the inadmissible ones dropped, and the topk-th best of the rest is the threshold (published too), or 0.
// count_first (uniform): some anchors may be no candidates, so fewer than kPlBoundRows may be left to choose from.
template <class Ctx, class Smem, class RowKey>
__device__ __forceinline__ uint64_t scan_anchor_threshold(const Ctx& c, const Smem& sm, const uint64_t (&mine)[kAnchorRows / PlaylistCfg::kBlock],
                                                          bool count_first, RowKey row_key, int& n_exact) {
    constexpr int kBlock = PlaylistCfg::kBlock, kPer = kAnchorRows / kBlock;
    static_assert(PlaylistCfg::kCandCap >= kAnchorRows / 2 && PlaylistCfg::kCandCap * 2 >= kPlBoundRows, "LDS reuse below");
    const int tid = c.tid, lane = c.lane;
    int n_cand = kPlBoundRows;   // anchors left to choose from: all of them without a filter
    if (count_first) {   // uniform
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
        const int64_t row = anchor_row(c.n, s_pick[tid]);
        const Row x = load_row(c.feats, row);   // from the matrix
        const bool x_pass = !c.active || filter_pass(x, c.active, c.buf->lo, c.buf->hi);   // (the filter tests the stored row)
        const uint64_t k = row_key(x, row);
        ++n_exact;
        key = playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + row)) || !x_pass ||
                      (c.labelled && !label_selected(sm.lmask, c.row_label[row])) || (c.rowset && !rowset_admits(c.rowset, c.flip, row))
                  ? 0ull
                  : k;
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

// The kernel's tail: the workgroup's n_exact into rows_exact, the last compaction, the ranked list of topk keys.
template <class Ctx, class Smem>
__device__ __forceinline__ void scan_finish(const Ctx& c, const Smem& sm, int n_exact, uint64_t* __restrict__ block_lists,
                                            unsigned long long* __restrict__ rows_exact) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    const int wave_exact = wave_inclusive_scan(n_exact);
    if (c.lane == 63 && wave_exact) atomicAdd(&sm.exact, wave_exact);
    __syncthreads();
    if (c.tid == 0 && rows_exact && sm.exact) atomicAdd(rows_exact, static_cast<unsigned long long>(sm.exact));
    if (sm.count > kRankCountMax && sm.count > c.topk)   // uniform
        compact_candidates<kBlock, PlaylistCfg::kCandPerThread>(sm.cand, &sm.count, c.topk, false, sm.sel);
    __syncthreads();
    block_rank_and_store<kBlock>(sm.cand, sm.count, block_lists + static_cast<int64_t>(blockIdx.x) * c.topk, c.topk);
}

// ---- the starting threshold: the best kPlBoundRows anchors by u, scored exactly (STARTING THRESHOLD above).  Returns the
// threshold key (published too), or 0.
__device__ __forceinline__ uint64_t playlist_anchor_bound(const PlaylistCtx& c, const PlaylistSmem& sm, const float (&u)[kDim], float un, int& n_exact) {
    constexpr int kBlock = PlaylistCfg::kBlock, kPer = kAnchorRows / kBlock;
    const int tid = c.tid;
    const int64_t n = c.n;
    const int n_anchor = n < kAnchorRows ? static_cast<int>(n) : kAnchorRows;   // (anchor i is row i below kAnchorRows rows)
    if (!(c.anchors && c.topk <= kPlBoundRows && n_anchor >= kPlBoundRows)) return 0ull;   // uniform
    uint64_t mine[kPer];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int i = r * kBlock + tid;
        Row a = load_row(c.anchors, static_cast<int64_t>(i));
        const bool a_pass = !c.active || filter_pass(a, c.active, c.buf->lo, c.buf->hi);   // (the filter tests the stored values)
        if (c.scaled) scale_row(a, sm.scale);   // (uniform)
        if (c.dist) {   // (uniform) DISTANCE: the anchors nearest to the centroid; a distance that is not finite is no candidate
            const float d = playlist_sqdist(&u, 1, a);   // (the chain's d2 against the centroid: K = 1 divides by 1.0f, exactly)
            mine[r] = i < n_anchor && d < __builtin_inff() ? pack_key(-d, static_cast<uint32_t>(i)) : 0ull;
        } else {
            mine[r] = i < n_anchor ? pack_key(cosine_score(u, un, a), static_cast<uint32_t>(i)) : 0ull;
        }
        if (!a_pass) mine[r] = 0ull;   // (only chooses: re-checked on the matrix's row)
        if (c.labelled && i < n_anchor && !label_selected(sm.lmask, c.row_label[anchor_row(n, i)])) mine[r] = 0ull;
    }
    return scan_anchor_threshold(c, sm, mine, c.active || c.labelled || c.dist,
                                 [&](const Row& x, int64_t row) { return playlist_row_key(c, sm, x, row); }, n_exact);
}

// One tile's streamed inputs of a lane: its quad of the replica, of the labels and of the side values.
struct PlaylistTile {
    HalfTile q8;
    uint2 labels;
    float4 side;
};

// The quad a lane reads of tile t: past the last quad it re-reads the last one.
__device__ __forceinline__ int64_t playlist_tile_quad(int64_t t, int tid, int64_t n_quads) {
    const int64_t quad = t * PlaylistCfg::kBlock + tid;
    return quad < n_quads ? quad : n_quads - 1;
}

// Loads what the launch streams of tile t into `d` (the rest keeps its value); replica, side: the cut's kind reads them (uniform).
// (Each load clamps its own quad: one clamped index held across the three branches costs the kernel two registers it does not have.)
__device__ __forceinline__ void playlist_load_tile(const PlaylistCtx& c, bool replica, bool side, int64_t n_quads, int64_t t, PlaylistTile& d) {
    if (replica) d.q8 = reinterpret_cast<const HalfTile*>(c.q8)[playlist_tile_quad(t, c.tid, n_quads)];   // (three uint4 to a quad)
    if (c.labelled) d.labels = c.labels4[playlist_tile_quad(t, c.tid, n_quads)];
    if (side) d.side = c.side4[playlist_tile_quad(t, c.tid, n_quads)];   // (the exact path reloads a row's prior in the chain loop)
}

// ---- the scan: this workgroup's tiles, candidates into sm.cand (thr: the starting threshold key, or 0)
__device__ __forceinline__ void playlist_scan_tiles(const PlaylistCtx& c, const PlaylistSmem& sm, const Q8Query& hq, PlaylistCut& cut, uint64_t thr, int& n_exact,
                                                    bool no_proof) {
    constexpr int kBlock = PlaylistCfg::kBlock;
    const int tid = c.tid, lane = c.lane;
    const int64_t n = c.n, n_quads = (n + 3) >> 2, tiles = (n_quads + kBlock - 1) / kBlock;
    playlist_cut_refresh(cut, thr);
    const bool counting = c.topk == 0;   // (uniform) BOUNDED above: n_exact counts the matches, nothing is appended, thr never moves
    // PROVEN IN (playlist_cut.hip.h, "BOUNDED"): the floor's own score is the image (thr + 1) >> 32; uniform, fixed for the launch
    const bool proving = counting && cut.kind == kPlCutPlain && !c.active && !no_proof;
    const int cut_hi = proving ? playlist_cut_proven(cut, ordered_to_score(static_cast<uint32_t>((thr + 1ull) >> 32))) : kPlCutNever;
    const int compact_at = scan_compact_at(c.topk);
    PlaylistTile cur = {};   // (zeros where nothing streams)
    const bool replica = cut.kind != kPlCutOff, side = cut.kind == kPlCutPrior || cut.kind == kPlCutDistance;   // what streams
    playlist_load_tile(c, replica, side, n_quads, blockIdx.x, cur);

    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform
        PlaylistTile nxt = cur;
        playlist_load_tile(c, replica, side, n_quads, t + gridDim.x, nxt);   // the next tile is in flight while this one is scored
        // (the quad's admissible mask stays written out here and in anyof_scan_tiles: as a function it moved anyof.hip.h's two kernels by 1 - 2 VGPRs)
        const int64_t quad = t * kBlock + tid;
        const int64_t r0 = quad * 4;
        const int64_t left = quad < n_quads ? n - r0 : 0;   // rows of the quad inside the shard
        uint32_t mask = left >= 4 ? 0xfu : (1u << static_cast<int>(left)) - 1u;
        if (c.rowset) {   // (uniform) ROW SETS: the quad's nibble, before anything else is done with its rows
            const int64_t q = playlist_tile_quad(t, tid, n_quads);
            mask &= ((static_cast<uint32_t>(c.rowset[q >> 1]) >> ((static_cast<uint32_t>(q) & 1u) * 4u)) ^ c.flip) & 0xfu;
        }
        if (c.labelled) {   // (uniform) the label test: it needs nothing but the label
            const int l4[4] = {static_cast<int16_t>(cur.labels.x & 0xffffu), static_cast<int16_t>(cur.labels.x >> 16),
                               static_cast<int16_t>(cur.labels.y & 0xffffu), static_cast<int16_t>(cur.labels.y >> 16)};
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4)
                if (!label_selected(sm.lmask, l4[u4])) mask &= ~(1u << u4);
        }
        if (cut.kind != kPlCutOff) {   // uniform
            int a[4];
            bool special[4];
            q8_dot4(hq, cur.q8, a, special);
            playlist_cut_apply(cut, mask, a, special, cur.side, cur.q8, sm.abar);
            if (proving) {   // (uniform) a row proven in matches unless it is excluded: counted here, its fp32 row never read
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4)
                    if ((mask & (1u << u4)) && !special[u4] && a[u4] >= cut_hi) {
                        mask &= ~(1u << u4);
                        n_exact += c.n_excl > 0 && playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + r0 + u4)) ? 0 : 1;
                    }
            }
        }
        scan_quad_filter(c, r0, counting, mask, n_exact);
        while (__ballot(mask != 0u)) {   // uniform
            const bool have = mask != 0u;
            const int64_t r = have ? r0 + __builtin_ctz(mask) : 0;
            const uint64_t row_key = playlist_row_key(c, sm, load_row(c.feats, r), r);
            n_exact += (have && !c.active && !counting) ? 1 : 0;   // (with a filter every row read was counted above)
            const uint64_t key = have ? row_key : 0ull;
            bool pass = key > thr;
            if (pass && c.n_excl > 0) pass = !playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + r));
            if (counting) n_exact += pass ? 1 : 0, pass = false;   // a match: counted, never listed
            scan_append(sm, lane, pass, key);
            mask &= mask - 1u;
        }
        thr = scan_exchange(c, sm, compact_at, thr);
        playlist_cut_refresh(cut, thr);
        cur = nxt;
    }
}

// ---- CANDIDATE LISTS: the gather, playlist_scan_tiles' sibling: the listed rows `cand[0..n_cand)` of this workgroup, candidates
// into sm.cand.  The threshold starts at 0; nothing of the cut is read.
// List entries of a thread per iteration, their rows in flight together.  The kernel sits on its budget
// of 128 VGPRs without scratch: 4 entries (48 row registers) and 3 spill, 2 fit; what is in flight per CU comes from its 1024 threads.
constexpr int kPlGatherPerThread = 2;
__device__ __forceinline__ void playlist_gather_rows(const PlaylistCtx& c, const PlaylistSmem& sm, const uint32_t* __restrict__ cand,
                                                     int64_t n_cand, uint64_t* __restrict__ entry_keys, int& n_exact) {
    constexpr int kBlock = PlaylistCfg::kBlock, kPer = kPlGatherPerThread;
    static_assert(kBlock * kPer <= PlaylistCfg::kTileRows, "an iteration appends at most a tile's worth of keys (kCandCap)");
    const int tid = c.tid, lane = c.lane;
    const int64_t chunks = (n_cand + kBlock * kPer - 1) / (kBlock * kPer);
    const bool score = c.topk == 0;   // (uniform) CANDIDATE SCORES: every entry's key to entry_keys, nothing selected
    uint64_t thr = 0ull;
    const int compact_at = scan_compact_at(c.topk);

    for (int64_t t = blockIdx.x; t < chunks; t += gridDim.x) {   // uniform
        const int64_t e0 = (t * kBlock + tid) * kPer;
        uint32_t row[kPer], mask = 0u;
        Row x[kPer];
#pragma unroll
        for (int v = 0; v < kPer; ++v) {
            row[v] = cand[e0 + v < n_cand ? e0 + v : n_cand - 1];
            if (e0 + v < n_cand) mask |= 1u << v;
        }
#pragma unroll
        for (int v = 0; v < kPer; ++v) x[v] = load_row(c.feats, static_cast<int64_t>(row[v]));   // requested together
        if (c.rowset) {   // (uniform) ROW SETS
#pragma unroll
            for (int v = 0; v < kPer; ++v)
                if (!rowset_admits(c.rowset, c.flip, static_cast<int64_t>(row[v]))) mask &= ~(1u << v);
        }
        if (c.labelled) {   // (uniform) the label, by row
#pragma unroll
            for (int v = 0; v < kPer; ++v)
                if (!label_selected(sm.lmask, c.row_label[row[v]])) mask &= ~(1u << v);
        }
        n_exact += __builtin_popcount(mask);   // every row that reaches the filter or the chains
        if (c.active) {   // (uniform) the filter on the stored rows
#pragma unroll
            for (int v = 0; v < kPer; ++v)
                if (!filter_pass(x[v], c.active, c.buf->lo, c.buf->hi)) mask &= ~(1u << v);
        }
#pragma unroll
        for (int v = 0; v < kPer; ++v) {   // (uniform) entry v of every thread (unrolled: x[v] is a register, never indexed)
            const bool have = (mask & (1u << v)) != 0u;
            const uint64_t row_key = playlist_row_key(c, sm, x[v], static_cast<int64_t>(row[v]));
            const uint64_t key = have ? row_key : 0ull;
            bool pass = key > thr;
            if (pass && c.n_excl > 0) pass = !playlist_excluded(sm.excl, c.n_excl, static_cast<uint32_t>(c.row_base + row[v]));
            if (score) {   // (uniform) entry e0 + v's word: its key, or 0 (thr stays 0, so every key was looked up in the exclusion list)
                if (e0 + v < n_cand) entry_keys[e0 + v] = pass ? key : 0ull;
                continue;
            }
            scan_append(sm, lane, pass, key);
        }
        if (score) continue;   // (uniform) nothing was appended: no barrier, no compaction, no threshold
        thr = scan_exchange(c, sm, compact_at, thr);
    }
}

// q8: the handle's 8-bit replica, or null (every row exact).  anchors: the anchor table, or null (no starting threshold).
// rows_exact: += the rows whose K chains this launch computed; with a filter, every fp32 row read (rejected ones included).
// labels: the shard's labels in row order, four int16 to a quad (read only where arg.labelled).
// priors: the shard's priors in row order, four fp32 to a quad (read only where arg.prior).
// norms: DISTANCE: the rows' norms in row order, four fp32 to a quad, or null (no pre-filter for this metric then).
__global__ __launch_bounds__(PlaylistCfg::kBlock, PlaylistCfg::kMinWaves) void playlist_scan_kernel(
    const float* __restrict__ feats, const uint4* __restrict__ q8, int64_t n, int64_t row_base, const PlaylistBuf* __restrict__ buf,
    PlaylistArg arg, const float* __restrict__ anchors, int topk, uint64_t* __restrict__ block_lists,
    unsigned long long* __restrict__ rows_exact, unsigned long long* __restrict__ shared_thr /* &buf->shared_thr */,
    const uint2* __restrict__ labels, const float4* __restrict__ priors, const float4* __restrict__ norms) {
    __shared__ uint64_t s_cand[PlaylistCfg::kCandCap];
    __shared__ SelectSmem s_sel;
    __shared__ int s_count, s_ok, s_exact;
    __shared__ unsigned long long s_shared;
    __shared__ float s_mem[kMaxPlaylist][kDim];
    __shared__ float s_qn[kMaxPlaylist], s_w[kMaxPlaylist], s_u[kDim];
    __shared__ uint32_t s_excl[kPlExcludeCap], s_lmask[kMaxLabels / 32];
    __shared__ __attribute__((aligned(16))) float s_scale[kDim], s_abar[kDim];
    const PlaylistSmem sm = {s_cand, s_sel, s_count, s_ok, s_exact, s_shared, s_mem, s_qn, s_w, s_u, s_excl, s_lmask, s_scale, s_abar};
    const bool dist = arg.metric == kPlDistance;
    const int tid = threadIdx.x;
    const PlaylistCtx c = {feats, anchors, n, row_base, buf, shared_thr, arg.k, arg.n_excl, topk, arg.active, arg.wsum, arg.prior_weight,
                           arg.by_row != 0, arg.labelled != 0, arg.prior != 0, dist, arg.scaled != 0, arg.metric == kPlJaccard,
                           reinterpret_cast<const int16_t*>(labels), labels,
                           reinterpret_cast<const float*>(priors), dist ? norms : priors, q8, arg.rowset, arg.rowset_flip, tid, tid & 63};
    float u[kDim], un;
    PlaylistCut cut;
    const Q8Query hq = playlist_prologue(c, sm, u, un, cut);
    int n_exact = 0;   // rows whose K chains this thread computed
    // (uniform) CANDIDATE LISTS: only the listed rows.  Marked unlikely: a non-null pointer test counts as likely, and the register
    // allocator then weighs the scan's loops below the gather's and moves the kernel's spilled SGPRs into them (docs/LAB_NOTES.md).
    if (__builtin_expect(arg.cand != nullptr, 0)) {
        playlist_gather_rows(c, sm, arg.cand, arg.n_cand, block_lists, n_exact);
    } else {
        uint64_t thr = 0ull;
        if (topk == 0) thr = buf->shared_thr;   // (uniform) BOUNDED above: the count launch starts, and stays, at the floor
        else if (cut.kind != kPlCutOff) thr = playlist_anchor_bound(c, sm, u, un, n_exact);   // uniform
        playlist_scan_tiles(c, sm, hq, cut, thr, n_exact, arg.n_cand != 0);   // (n_cand without a list: BOUNDED above, the A/B knob)
    }

    scan_finish(c, sm, n_exact, block_lists, rows_exact);
}

}  // namespace mi355
