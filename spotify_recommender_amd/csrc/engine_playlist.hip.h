// engine_playlist.hip.h — PLAYLISTS on the single-device handle (include/mi355rec_diag.h, "PLAYLISTS"): the top-N rows by
// the mean of their scores against up to 32 member queries, an exclusion list left out.  One playlist_scan_kernel launch
// (playlist.hip.h), then the merge of merge.hip.h into the handle's pinned result slots and completion word, between
// sync_begin and sync_finish (engine_sync.hip.h) as sync_label_query does.  No state beyond a small per-handle buffer for the call's inputs, allocated by the first call.
// Every call of the family (filtered, weighted, diversified, capped; by value or by row) is one mi355playlist::Request
// (playlist_request.h) through sync_playlist_query; the exported functions only fill it.  An ANY-OF request (metric kAnyOf) takes the
// same path with anyof_scan_kernel (anyof.hip.h) at the launch and, where out_member is asked for, its attribution launch after the merge.
// A BOUNDED request (Request::bounded) takes the same path with one more launch ahead of the scan: playlist_scan_kernel's count form
// (topk == 0 without a list), whose total comes back through a pinned word; sync_playlist_query then cuts the merged results at the floor.
// (Part of mi355rec.hip's translation unit, included after engine_labels.hip.h.)
#pragma once

#include <algorithm>

#include "anyof.hip.h"
#include "candidates.h"
#include "engine_labels.hip.h"
#include "engine_rowset.hip.h"
#include "playlist.hip.h"
#include "playlist_request.h"

// What the first playlist call of a handle allocates.
struct mi355rec_playlist {
    PlaylistBuf* d_buf = nullptr;           // the call's members / member rows and excluded ids on the device ...
    PlaylistBuf* h_buf = nullptr;           // ... staged here (pinned)
    unsigned long long* d_exact = nullptr;  // rows whose K chains were computed, since the first call (mi355rec_playlist_counters)
    int grid_cap = 1;                       // workgroups of a launch at most (occupancy x CUs, and the handle's list slots)
    // DIVERSIFIED TOP-N (engine_diverse.hip.h), allocated by the first such call:
    float* h_mmr = nullptr;                 // the picks' mmr values: pinned, mapped, written by mmr_rerank_kernel itself ...
    float* hd_mmr = nullptr;                // ... at this device-side address
    float* d_rows = nullptr;                // kMaxTopK rows: a pool passed by value, or the rows mi355rec_fetch_rows gathers
    // GROUP CAPS (engine_diverse.hip.h):
    int* h_pool_rows = nullptr;             // P' of the last capped call: one more word of the pinned h_mmr allocation ...
    int* hd_pool_rows = nullptr;            // ... at this device-side address
    int32_t* d_pool_groups = nullptr;       // kMaxTopK groups: those of a pool passed by value, in pool order
    // DISTANCE REQUESTS (playlist.hip.h, "DISTANCE"): |x| of every row in local row order, padded to a whole quad, 4 B per row.
    // Built by the handle's first distance request that scans the 8-bit replica (q8_build_kernel with a null replica pointer, on
    // the handle's stream) and dropped by mi355rec_rebuild_replica: a snapshot of the rows, as the replica is.  It belongs to
    // THIS handle, not to RowSide: a lane builds and holds its own, so no lane ever builds under another lane's launch.
    float* d_norms = nullptr;
    bool norms_built = false;               // the build has been enqueued on the handle's stream: only then may a scan read d_norms
    // CANDIDATE LISTS (playlist.hip.h, "CANDIDATE LISTS"): a request's listed rows of this shard, reduced on the host (candidates.h)
    // into the pinned h_cand and copied to d_cand on the handle's stream ahead of the launch.  Both hold cand_cap entries and grow on
    // demand, before the call is begun.
    uint32_t* h_cand = nullptr;
    uint32_t* d_cand = nullptr;
    int64_t cand_cap = 0;
    int64_t cand_requests = 0, cand_rows = 0;   // mi355rec_candidates_counters
    // CANDIDATE SCORES (playlist.hip.h, "CANDIDATE SCORES"): the key of every entry of d_cand, stored by the scoring launch, copied back
    // into the pinned h_cand_keys on the handle's stream.  Both hold cand_key_cap entries and grow with the list's buffers.
    uint64_t* h_cand_keys = nullptr;
    uint64_t* d_cand_keys = nullptr;
    int64_t cand_key_cap = 0;
    std::vector<int64_t> cand_pos;              // list order -> entry of d_cand (candidates.h, positions) ...
    int64_t cand_entries = 0;                   // ... of which the scoring launch was given this many
    // ANY-OF REQUESTS (anyof.hip.h, "ATTRIBUTION"): a(x) of the merged result's rows, stored by the attribution launch, copied back into
    // the pinned h_member on the handle's stream.  kMaxTopK entries each, allocated with the buffers above.
    int32_t* d_member = nullptr;
    int32_t* h_member = nullptr;
    // BOUNDED REQUESTS (playlist.hip.h, "BOUNDED"): the count launch's total word (its `rows_exact`): zeroed on the handle's stream
    // ahead of the launch, copied into the pinned h_total behind it; the call's completion covers both.
    unsigned long long* d_total = nullptr;
    unsigned long long* h_total = nullptr;
    bool counted = false;                       // the last playlist_launch enqueued a count launch: h_total is this call's
};

namespace {

using mi355playlist::Outputs;
using mi355playlist::Request;
using mi355playlist::request;

// mi355rec_set_priors: the priors' own checks and upload (replace_side, engine_labels.hip.h, does the rest).  The device
// array is padded with +0.0f to a whole quad (playlist_scan_kernel loads a quad's four priors at once).
int set_priors_common(mi355rec* h, const float* priors_host, int64_t n, bool group_ok) {
    return replace_side(h, &RowSide::d_priors, "priors", group_ok, priors_host != nullptr, [&](float** fresh) {
        if (n != h->n) return fail(h, MI355REC_ERR_INVALID_ARG, "%lld priors for a handle of %lld rows", (long long)n, (long long)h->n);
        const int64_t bad = mi355playlist::first_bad_prior(priors_host, n);
        if (bad >= 0)
            return fail(h, MI355REC_ERR_INVALID_ARG, "prior %g of row %lld: a prior is finite with |p| <= 1",
                        static_cast<double>(priors_host[bad]), (long long)bad);
        // (an empty shard keeps a one-quad array: "has priors" is a non-null pointer)
        const size_t padded = static_cast<size_t>(n > 0 ? (n + 3) / 4 * 4 : 4);
        hipError_t e = hipMalloc(fresh, sizeof(float) * padded);
        if (e == hipSuccess) e = hipMemset(*fresh, 0, sizeof(float) * padded);
        if (e == hipSuccess && n > 0) e = hipMemcpy(*fresh, priors_host, sizeof(float) * static_cast<size_t>(n), hipMemcpyHostToDevice);
        if (e == hipSuccess) return static_cast<int>(MI355REC_OK);
        if (*fresh) (void)hipFree(*fresh);
        return fail(h, e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, "the priors (%lld rows): %s",
                    (long long)n, hipGetErrorString(e));
    });
}

// "MANHATTAN REQUESTS": the most members for which the launch takes the 8-bit pre-filter (playlist_cut.hip.h, "MANHATTAN"): its
// arithmetic grows with K as the chains' does, only its bytes do not.  Measured on an MI355X at 10 M uniform rows, top-100, with
// the cut at every K (profiles/r23_manhattan_cut_every_k.json: the experiments build with MI355REC_EXP_L1_CUT_MAX_K=32), p50 on a
// handle with the replica / on one without: K = 1: 97.7 / 192.9 us, K = 3: 113.6 / 194.8, K = 10: 185.4 / 210.4, K = 32: 416.1 /
// 270.1 (300-cluster sorted catalogue: 99.5 / 203.1, 109.8 / 201.3, 169.0 / 212.9, 347.9 / 268.9).  Both grow linearly in K
// (about 10 us and under 3 us per member) and cross near K = 12; K = 10 is the largest K measured at which the cut wins, so it
// is on up to there.
constexpr int kL1CutMaxK = 10;
constexpr int kPlMinTilesPerWg = 8;   // with the pre-filter: a workgroup scans >= 8 tiles (its anchor bound paid for, its own threshold tight)

void free_playlist(mi355rec_playlist* P) {
    if (!P) return;
    if (P->d_buf) (void)hipFree(P->d_buf);
    if (P->d_exact) (void)hipFree(P->d_exact);
    if (P->h_buf) (void)hipHostFree(P->h_buf);
    if (P->h_mmr) (void)hipHostFree(P->h_mmr);
    if (P->d_rows) (void)hipFree(P->d_rows);
    if (P->d_pool_groups) (void)hipFree(P->d_pool_groups);
    if (P->d_norms) (void)hipFree(P->d_norms);
    if (P->h_cand) (void)hipHostFree(P->h_cand);
    if (P->d_cand) (void)hipFree(P->d_cand);
    if (P->h_cand_keys) (void)hipHostFree(P->h_cand_keys);
    if (P->d_cand_keys) (void)hipFree(P->d_cand_keys);
    if (P->d_member) (void)hipFree(P->d_member);
    if (P->h_member) (void)hipHostFree(P->h_member);
    if (P->d_total) (void)hipFree(P->d_total);
    if (P->h_total) (void)hipHostFree(P->h_total);
    delete P;
}

int ensure_playlist(mi355rec* h) {
    if (h->playlist) return MI355REC_OK;
    mi355rec_playlist* P = new (std::nothrow) mi355rec_playlist();
    if (!P) return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for the playlist buffers");
    auto failed = [&](hipError_t e, const char* what) {
        free_playlist(P);
        return fail(h, e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMalloc(&P->d_buf, sizeof(PlaylistBuf))) != hipSuccess) return failed(e, "hipMalloc(playlist buffer)");
    if ((e = hipHostMalloc(&P->h_buf, sizeof(PlaylistBuf), hipHostMallocDefault)) != hipSuccess) return failed(e, "hipHostMalloc(playlist buffer)");
    if ((e = hipMalloc(&P->d_exact, sizeof(unsigned long long))) != hipSuccess) return failed(e, "hipMalloc(playlist counter)");
    if ((e = hipMemset(P->d_exact, 0, sizeof(unsigned long long))) != hipSuccess) return failed(e, "hipMemset(playlist counter)");
    if ((e = hipMalloc(&P->d_member, sizeof(int32_t) * kMaxTopK)) != hipSuccess) return failed(e, "hipMalloc(any-of members)");
    if ((e = hipHostMalloc(&P->h_member, sizeof(int32_t) * kMaxTopK, hipHostMallocDefault)) != hipSuccess) return failed(e, "hipHostMalloc(any-of members)");
    if ((e = hipMalloc(&P->d_total, sizeof(unsigned long long))) != hipSuccess) return failed(e, "hipMalloc(bounded total)");
    if ((e = hipHostMalloc(&P->h_total, sizeof(unsigned long long), hipHostMallocDefault)) != hipSuccess) return failed(e, "hipHostMalloc(bounded total)");
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, playlist_scan_kernel, PlaylistCfg::kBlock, 0) != hipSuccess || occ < 1) occ = 1;
    (void)hipGetLastError();
    const int lists = most(h, &ScanGeom::grid);   // d_block_lists holds this many lists of kMaxTopK keys (create)
    P->grid_cap = h->cus * occ;
    if (P->grid_cap > lists) P->grid_cap = lists;
    if (P->grid_cap > kMergeMaxLists) P->grid_cap = kMergeMaxLists;
    if (P->grid_cap < 1) P->grid_cap = 1;
    h->playlist = P;
    return MI355REC_OK;
}

// CANDIDATE LISTS: room for `want` list entries in h_cand and d_cand (the previous call on this handle has completed: nothing reads
// the old buffers).  A failure leaves the handle without them; the next request allocates again.
// keys: CANDIDATE SCORES: room for `want` keys in h_cand_keys and d_cand_keys as well (8 B per entry, at most 8 MB), under the same rules.
template <typename T>
hipError_t grow_candidates(T** host, T** dev, int64_t* have, int64_t want) {
    if (want <= *have) return hipSuccess;
    int64_t cap = *have > 0 ? *have : 4096;
    while (cap < want) cap *= 2;
    if (*host) (void)hipHostFree(*host);
    if (*dev) (void)hipFree(*dev);
    *host = *dev = nullptr;
    *have = 0;
    hipError_t e = hipHostMalloc(host, sizeof(T) * static_cast<size_t>(cap), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(dev, sizeof(T) * static_cast<size_t>(cap));
    if (e == hipSuccess) {
        *have = cap;
        return hipSuccess;
    }
    if (*host) (void)hipHostFree(*host);
    *host = *dev = nullptr;
    (void)hipGetLastError();
    return e;
}

int ensure_candidates(mi355rec* h, mi355rec_playlist* P, int64_t want, bool keys = false) {
    hipError_t e = grow_candidates(&P->h_cand, &P->d_cand, &P->cand_cap, want);
    if (e == hipSuccess && keys) e = grow_candidates(&P->h_cand_keys, &P->d_cand_keys, &P->cand_key_cap, want);
    if (e == hipSuccess) return MI355REC_OK;
    return fail(h, e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, "the candidate list (%lld ids): %s", (long long)want,
                hipGetErrorString(e));
}

// One call of the playlist family (playlist_request.h), synchronously.  r.members: k x 12 floats on the host, or null with
// r.rows (k rows of this shard, excluded by their global ids).  r.exclude[0..n_exclude): global ids, any order, duplicates
// allowed; ids of other shards match nothing here.  r.filter: null, or the feature filter (include/mi355rec_diag.h, "FEATURE
// FILTERS"); null and active == 0 launch exactly the unfiltered call.  r.weights: null, or k signed weights
// (include/mi355rec_diag.h, "WEIGHTED PLAYLISTS"); null launches the same kernel with every weight 1.0f and W = k, which is the
// plain mean bit for bit.  r.labels: null, or the label set (include/mi355rec_diag.h, "PLAYLIST REQUESTS"): only rows whose label
// (mi355rec_set_labels) is in it are admissible; null launches exactly the call without labels.
//
// playlist_launch is the call up to and including its scan launch: the checks, sync_begin (engine_sync.hip.h), the staging
// and playlist_scan_kernel, which leaves `*grid` lists of `ss->eff` = min(r.scan_topn(), rows left after the exclusion list)
// keys in h->d_block_lists.  ss->eff == 0: nothing is left to return and nothing was begun or launched.  What follows the
// scan is sync_playlist_query's: the plain call merges into the result slots; the diversified one merges, re-ranks and waits
// once (engine_diverse.hip.h).
int playlist_launch(mi355rec* h, const Request& r, int max_exclude, SyncSlots* ss, int* grid_out) {
    *ss = SyncSlots();
    *grid_out = 0;
    char why[128];
    if (mi355playlist::invalid_playlist(r, h->n, static_cast<int64_t>(UINT32_MAX) + 1, max_exclude, why, sizeof why))
        return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    const int k = r.k;
    DeviceGuard guard(h->device);
    int rc = ensure_playlist(h);
    if (rc) return rc;
    mi355rec_playlist* P = h->playlist;
    PlaylistBuf* b = P->h_buf;
    P->counted = false;
    // the excluded rows of this shard: sorted, distinct, as uint32 global ids
    int n_excl = 0;
    for (int i = 0; i < r.n_exclude; ++i)
        if (r.exclude[i] >= h->row_base && r.exclude[i] < h->row_base + h->n) b->excl[n_excl++] = static_cast<uint32_t>(r.exclude[i]);
    if (r.rows)
        for (int m = 0; m < k; ++m) b->excl[n_excl++] = static_cast<uint32_t>(h->row_base + r.rows[m]);
    std::sort(b->excl, b->excl + n_excl);
    n_excl = static_cast<int>(std::unique(b->excl, b->excl + n_excl) - b->excl);
    int64_t avail = h->n - n_excl;
    // the label set ("PLAYLIST REQUESTS"): at most the selected rows are left (host offsets); nothing selected: no launch
    const mi355rec_labels* L = nullptr;
    if (r.n_labels > 0) {
        L = h->side->labels;
        if (!L) return fail(h, MI355REC_ERR_INVALID_ARG, "this handle has no labels (mi355rec_set_labels)");
        LabelMask mask;
        int64_t selected = 0, label_tiles = 0;
        rc = label_mask(h, L, r.labels, r.n_labels, &mask, &selected, &label_tiles);
        if (rc) return rc;
        std::memcpy(b->label_mask, mask.w, sizeof b->label_mask);
        if (selected < avail) avail = selected;
    }
    // the row set ("ROW SETS"): this handle's copy of the bitmap; at most the rows it admits are left (an upper bound, as `selected`
    // is).  A set that rejects no row of this shard launches exactly the call without it.
    const uint8_t* set_bits = nullptr;
    if (r.rowset) {
        const mi355rowset::Part* part = rowset_part(h, r.rowset);
        if (!part) return fail(h, MI355REC_ERR_INVALID_ARG, "row set of another handle");
        const int64_t admitted = r.rowset_only ? part->count : h->n - part->count;
        if (admitted < avail) avail = admitted;
        if (admitted < h->n) set_bits = part->d_bits;
    }
    // the candidate list ("CANDIDATE LISTS"): this shard's listed rows, sorted and distinct, into the pinned buffer; at most they
    // are left.  The launch below then gathers them and reads nothing else of the catalogue.
    int64_t n_cand = 0;
    if (r.listed) {
        if (r.n_candidates > 0) {
            rc = ensure_candidates(h, P, r.n_candidates, r.score);
            if (rc) return rc;
            // (one pass over the ids: the range check of a list that comes unchecked, the shard's rows, the ascending test)
            const mi355cand::Reduced red =
                mi355cand::reduce(r.candidates, r.n_candidates, h->row_base, h->row_base + h->n, P->h_cand, r.candidates_id_end);
            if (red.bad >= 0) {
                mi355cand::bad_id_message(r.candidates[red.bad], r.candidates_id_end, why, sizeof why);
                return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
            }
            n_cand = red.count;
            if (r.score) {   // "CANDIDATE SCORES": where each list position finds its entry
                P->cand_entries = n_cand;
                P->cand_pos.resize(static_cast<size_t>(r.n_candidates));
                mi355cand::positions(r.candidates, r.n_candidates, h->row_base, h->row_base + h->n, P->h_cand, red, P->cand_pos.data());
            }
        }
        if (n_cand < avail) avail = n_cand;
    }
    // the prior ("ROW PRIORS"): checked whenever the request carries one; beta == 0 then launches exactly the call without it
    const float* pri = nullptr;
    if (r.prior) {
        pri = h->side->d_priors;
        if (!pri) return fail(h, MI355REC_ERR_INVALID_ARG, "this handle has no priors (mi355rec_set_priors)");
        if (r.prior_weight == 0.0f) pri = nullptr;
    }
    ++h->playlist_queries;
    const int eff = static_cast<int64_t>(r.scan_topn()) < avail ? r.scan_topn() : static_cast<int>(avail);
    // "BOUNDED REQUESTS": the count launch goes whenever a row could be admissible, whatever topn is
    const bool count_launch = r.bounded && avail > 0;
    if (eff <= 0 && !count_launch) return MI355REC_OK;   // nothing left to return: nothing to launch
    // "CANDIDATE SCORES": the launch selects nothing (topk == 0 is the kernel's score mode) and needs no result slot
    const int topk = r.score ? 0 : eff;
    PlaylistArg arg;
    arg.k = k;
    arg.n_excl = n_excl;
    arg.by_row = r.rows ? 1 : 0;
    arg.active = r.filter ? r.filter->active : 0u;
    arg.wsum = r.weights ? mi355weights::sum_abs(r.weights, k) : static_cast<float>(k);
    arg.labelled = L ? 1 : 0;
    arg.prior = pri ? 1 : 0;
    arg.prior_weight = pri ? r.prior_weight : 0.0f;
    const bool jaccard = r.metric == mi355playlist::kJaccard;
    arg.metric = r.metric == mi355playlist::kDistance ? kPlDistance : jaccard ? kPlJaccard : kPlCosine;
    arg.rowset = set_bits;
    arg.rowset_flip = set_bits && !r.rowset_only ? 0xfu : 0u;   // EXCLUDE: a set bit clears the row; ONLY: a clear bit does
    arg.cand = r.listed ? P->d_cand : nullptr;   // (eff > 0: the list has an entry)
    arg.n_cand = n_cand;
    arg.scaled = r.scales ? 1 : 0;   // "FEATURE SCALES" (every scale 1.0f has become null scales: the unscaled launch)
    for (int j = 0; j < kDim; ++j) b->scales[j] = r.scales ? r.scales[j] : 1.0f;
    for (int m = 0; m < k; ++m) b->weights[m] = r.weights ? r.weights[m] : 1.0f;
    if (arg.active) {
        std::memcpy(b->lo, r.filter->lo, sizeof b->lo);
        std::memcpy(b->hi, r.filter->hi, sizeof b->hi);
    }
    if (r.rows) std::memcpy(b->rows, r.rows, sizeof(int64_t) * static_cast<size_t>(k));
    else std::memcpy(b->members, r.members, sizeof(float) * kDim * static_cast<size_t>(k));
    // "DISTANCE REQUESTS": the rows' norms, once per handle (and per rebuild).  Allocated before the call is begun: a failure
    // here leaves nothing begun and nothing staged.
    // (a candidate list gathers: no replica, no anchors, no norms, so the cut is off and every listed row takes the exact chain)
    const uint4* q8 = !r.listed && use_q8(h) ? h->d_q8 : nullptr;
    // "MANHATTAN REQUESTS": the same norms; above kL1CutMaxK members the launch gets no replica (the cut loses to the chains there)
    const bool manhattan = r.metric == mi355playlist::kManhattan;
    int l1_cut_max_k = kL1CutMaxK;
    MI355REC_EXP_INT(l1_cut_max_k, "MI355REC_EXP_L1_CUT_MAX_K", 0, MI355REC_MAX_PLAYLIST);   // (experiments build only: tools/run_manhattan.py)
    if (manhattan && k > l1_cut_max_k) q8 = nullptr;
    // "JACCARD REQUESTS": no pre-filter: every row takes the chains, whatever the handle holds (playlist.hip.h, JACCARD)
    if (jaccard) q8 = nullptr;
    const int64_t n_quads4 = (h->n + 3) / 4 * 4;
    // (a scaled distance request takes the exact path: the norms are those of the unscaled rows, it is launched with null norms)
    const bool scan_norms = q8 && ((arg.metric == kPlDistance && !arg.scaled) || manhattan);
    const bool fresh_norms = scan_norms && !P->norms_built;
    if (fresh_norms && !P->d_norms) {   // (an earlier call that failed before its build was enqueued has left the allocation)
        const hipError_t e = hipMalloc(&P->d_norms, sizeof(float) * static_cast<size_t>(n_quads4));
        if (e != hipSuccess) {
            P->d_norms = nullptr;
            (void)hipGetLastError();
            return fail(h, e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, "the row norms (%lld rows): %s",
                        (long long)h->n, hipGetErrorString(e));
        }
    }
    // "ANY-OF REQUESTS": with out_member the merge is not the call's last launch (the attribution follows): it does not notify
    const bool anyof = r.metric == mi355playlist::kAnyOf;
    rc = sync_begin(h, topk, 1, !(anyof && r.attribute), ss);
    if (rc) return rc;
    // "BOUNDED REQUESTS": the floor, where every other call stages 0.  The count launch starts from it and never moves it; the top-N
    // launch behind it is SEEDED with it: every workgroup adopts the word after its first tile, which is sound (only keys above the
    // floor are wanted; sync_playlist_query cuts whatever the first tiles let through) and costs nothing: one staging serves both.  Its
    // lists may then hold fewer than `eff` keys, as a filtered call's already may: block_rank_and_store pads a short list with 0
    // keys, the merge sorts them last and sync_finish counts the ids >= 0.
    b->shared_thr = r.bounded ? r.floor_thr : 0ull;
    // (the staging buffer is free: the previous call on this handle has completed)
    const size_t bytes = offsetof(PlaylistBuf, excl) + sizeof(uint32_t) * static_cast<size_t>(n_excl);
    HIP_TRY(h, hipMemcpyAsync(P->d_buf, b, bytes, hipMemcpyHostToDevice, h->stream));
    if (fresh_norms) {   // (on the handle's stream, ahead of the scan that reads them)
        hipLaunchKernelGGL(q8_build_kernel, dim3(static_cast<unsigned>((n_quads4 + 255) / 256)), dim3(256), 0, h->stream, h->d_feats, h->n,
                           n_quads4, static_cast<uint32_t*>(nullptr), P->d_norms, static_cast<const int32_t*>(nullptr),
                           static_cast<const float*>(nullptr), 0, static_cast<int32_t*>(nullptr),
                           static_cast<const int64_t*>(nullptr), static_cast<const int64_t*>(nullptr), static_cast<uint2*>(nullptr), static_cast<float*>(nullptr));
        HIP_TRY(h, hipGetLastError());
        P->norms_built = true;   // (only now: every exit above leaves an array that the next request builds)
    }
    if (r.listed) {   // (on the handle's stream, ahead of the launch that reads them)
        HIP_TRY(h, hipMemcpyAsync(P->d_cand, P->h_cand, sizeof(uint32_t) * static_cast<size_t>(n_cand), hipMemcpyHostToDevice, h->stream));
        ++P->cand_requests;
        P->cand_rows += n_cand;
    }
    const int64_t tiles = ((h->n + 3) / 4 + PlaylistCfg::kBlock - 1) / PlaylistCfg::kBlock;
    int64_t want_grid = q8 ? (tiles + kPlMinTilesPerWg - 1) / kPlMinTilesPerWg : tiles;
    if (r.listed) want_grid = (n_cand + PlaylistCfg::kBlock * kPlGatherPerThread - 1) / (PlaylistCfg::kBlock * kPlGatherPerThread);
    if (want_grid > P->grid_cap) want_grid = P->grid_cap;
    if (want_grid < 1) want_grid = 1;
    const int grid = static_cast<int>(want_grid);
    // what every launch below passes: the call's staged inputs and the word inside them, the shard's labels, the rows' norms
    const PlaylistBuf* const d_buf = P->d_buf;
    unsigned long long* const shared_thr = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(P->d_buf) + offsetof(PlaylistBuf, shared_thr));
    const uint2* const labels = reinterpret_cast<const uint2*>(L ? L->d_row_labels : nullptr);
    const float4* const norms = reinterpret_cast<const float4*>(scan_norms ? P->d_norms : nullptr);
    const float* const anchors = h->d_anchor;
    if (count_launch) {   // "BOUNDED REQUESTS": the count form: topk == 0 without a list, the total word as rows_exact; AHEAD of the
        // top-N launch, which raises shared_thr above the floor
        HIP_TRY(h, hipMemsetAsync(P->d_total, 0, sizeof(unsigned long long), h->stream));
        PlaylistArg count_arg = arg;
        // (experiments build only: tools/run_bounded.py's A/B of the proven-in shortcut; n_cand means nothing else without a list)
        if (MI355REC_EXP_FLAG("MI355REC_EXP_NO_PROVEN_IN")) count_arg.n_cand = 1;
        hipLaunchKernelGGL(playlist_scan_kernel, dim3(grid), dim3(PlaylistCfg::kBlock), 0, h->stream, h->d_feats, q8, h->n, h->row_base, d_buf,
                           count_arg, static_cast<const float*>(nullptr), 0, h->d_block_lists, P->d_total, shared_thr, labels,
                           reinterpret_cast<const float4*>(pri), norms);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(P->h_total, P->d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        P->counted = true;
        if (topk == 0) return MI355REC_OK;   // count only (or nothing to list): *grid_out stays 0
    }
    // "MANHATTAN REQUESTS", "ANY-OF REQUESTS": their own kernels (anyof.hip.h), this launch's geometry, inputs and lists
    const AnyofArg any = {k, n_excl, arg.by_row, arg.active, arg.labelled, arg.rowset, arg.rowset_flip, 0};
    if (manhattan) {
        LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, manhattan_scan_kernel, dim3(grid), dim3(PlaylistCfg::kBlock), h->stream,
                     h->d_feats, q8, h->n, h->row_base, d_buf, any, anchors, topk, h->d_block_lists, P->d_exact, shared_thr, labels, norms);
    } else if (anyof) {
        LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, anyof_scan_kernel, dim3(grid), dim3(PlaylistCfg::kBlock), h->stream,
                     h->d_feats, q8, h->n, h->row_base, d_buf, any, anchors, topk, h->d_block_lists, P->d_exact, shared_thr, labels,
                     static_cast<const uint64_t*>(nullptr), static_cast<int32_t*>(nullptr));
    } else {
        LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, playlist_scan_kernel, dim3(grid), dim3(PlaylistCfg::kBlock), h->stream,
                     h->d_feats, q8, h->n, h->row_base, d_buf, arg, r.listed ? nullptr : anchors, topk,
                     r.score ? P->d_cand_keys : h->d_block_lists, P->d_exact, shared_thr, labels, reinterpret_cast<const float4*>(pri), norms);
    }
    HIP_TRY(h, hipGetLastError());
    *grid_out = grid;
    return MI355REC_OK;
}

// "ANY-OF REQUESTS", ATTRIBUTION (anyof.hip.h): the same kernel once more over the `eff` merged keys in h->d_keys (the call's inputs
// are still staged in P->d_buf), one thread per result row, then the copy of the member indices into pinned memory: both on the
// handle's stream, behind the merge.
int anyof_attribute(mi355rec* h, const Request& r, int eff) {
    mi355rec_playlist* P = h->playlist;
    const AnyofArg any = {r.k, 0, r.rows ? 1 : 0, 0u, 0, nullptr, 0u, eff};
    hipLaunchKernelGGL(anyof_scan_kernel, dim3((eff + PlaylistCfg::kBlock - 1) / PlaylistCfg::kBlock), dim3(PlaylistCfg::kBlock), 0, h->stream,
                       h->d_feats, static_cast<const uint4*>(nullptr), h->n, h->row_base, static_cast<const PlaylistBuf*>(P->d_buf), any,
                       static_cast<const float*>(nullptr), 0, static_cast<uint64_t*>(nullptr), static_cast<unsigned long long*>(nullptr),
                       static_cast<unsigned long long*>(nullptr), static_cast<const uint2*>(nullptr), static_cast<const uint64_t*>(h->d_keys),
                       P->d_member);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(P->h_member, P->d_member, sizeof(int32_t) * static_cast<size_t>(eff), hipMemcpyDeviceToHost, h->stream));
    return MI355REC_OK;
}

// (engine_diverse.hip.h, included after this file: what a diversified call adds to the path)
int check_diverse(mi355rec* h, const Request& r);
int ensure_diverse(mi355rec* h);
int rerank_and_wait(mi355rec* h, const Request& r, const Outputs& out, SyncSlots ss, int pool, bool staged);

// The one synchronous path of the family.  max_exclude: kMaxExclude for the exported calls, kPlExcludeCap for the node's.
int sync_playlist_query(mi355rec* h, const Request& r, const Outputs& out, int max_exclude = kMaxExclude) {
    if (!h || !(r.members || r.rows) || !(out.idx || (r.bounded && r.topn == 0)) || (r.bounded && !out.total))
        return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    int rc = r.diverse ? check_diverse(h, r) : MI355REC_OK;
    if (rc) return rc;
    if (out.pool_rows) *out.pool_rows = 0;
    DeviceGuard guard(h->device);
    SyncSlots ss;
    int grid = 0;
    rc = playlist_launch(h, r, max_exclude, &ss, &grid);
    if (rc) return rc;
    const int eff = ss.eff;
    if (r.bounded && grid == 0) {   // "BOUNDED REQUESTS": no top-N launch: the count launch alone (wait for its total), or nothing at all
        *out.total = 0;
        if (h->playlist->counted) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            *out.total = static_cast<int64_t>(*h->playlist->h_total);
        }
        if (r.topn > 0) mi355playlist::pad(out, 0, r.topn, 0);
        else if (out.count) *out.count = 0;
        return MI355REC_OK;
    }
    if (eff <= 0) {
        mi355playlist::pad(out, 0, r.topn, 0);
        return MI355REC_OK;
    }
    // one round: the results always fit the pinned slots and the call's last launch raises the completion word
    static_assert(kMaxTopK <= kDirectResultSlots, "a playlist call has no copy-back branch");
    if (r.diverse) {   // the pool never leaves the device: no ids or scores are unpacked, the re-rank stores the picks
        rc = ensure_diverse(h);
        if (rc) return rc;
        rc = enqueue_merge(h, h->d_block_lists, grid, eff, eff, h->d_keys, nullptr, nullptr, h->stream);
        if (rc) return rc;
        return rerank_and_wait(h, r, out, ss, eff, false);
    }
    rc = enqueue_merge(h, h->d_block_lists, grid, eff, eff, h->d_keys, ss.idx, ss.score, h->stream, ss.want);
    if (rc) return rc;
    if (r.metric == mi355playlist::kAnyOf && r.attribute) {   // "ANY-OF REQUESTS": a(x) of the merged rows, ahead of the copy back
        rc = anyof_attribute(h, r, eff);
        if (rc) return rc;
    }
    rc = sync_finish(h, ss, r.topn, out.idx, out.score, out.count);
    if (rc == MI355REC_OK && r.bounded) {   // "BOUNDED REQUESTS": the total (copied ahead of the merge that was waited for), the cut at the floor
        *out.total = static_cast<int64_t>(*h->playlist->h_total);
        const int matched = mi355playlist::bounded_cut(r, h->h_idx, h->h_score, eff);
        mi355playlist::pad(out, matched, r.topn, matched);
    }
    if (rc == MI355REC_OK && out.member)   // (the stream has been waited for: ss.want == 0 with an attribution)
        for (int i = 0; i < r.topn; ++i) out.member[i] = i < eff && out.idx[i] >= 0 ? h->playlist->h_member[i] : -1;
    if (rc == MI355REC_OK && r.report_distance) mi355playlist::scores_to_distances(out, r.topn, r.metric);   // "DISTANCE REQUESTS": -m to sqrtf(m) ("MANHATTAN": to m)
    return rc;
}

// "CANDIDATE SCORES": the same request with r.score: the gather launch stores every entry's key and selects nothing, no merge
// follows; the keys come back through the pinned buffer and are unpacked in list order (P->cand_pos).  No launch (no list entry of
// this shard, or no row the request could admit): every candidate is inadmissible.
int sync_playlist_scores(mi355rec* h, const Request& r, const mi355playlist::ScoreOutputs& out, int max_exclude = kMaxExclude) {
    if (!h || !(r.members || r.rows) || !out.value) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    DeviceGuard guard(h->device);
    SyncSlots ss;
    int grid = 0;
    int rc = playlist_launch(h, r, max_exclude, &ss, &grid);
    if (rc) return rc;
    if (grid == 0) {
        for (int64_t i = 0; i < r.n_candidates; ++i) mi355playlist::score_none(out, i);
        return MI355REC_OK;
    }
    mi355rec_playlist* P = h->playlist;
    rc = sync_finish_buffer(h, P->h_cand_keys, P->d_cand_keys, sizeof(uint64_t) * static_cast<size_t>(P->cand_entries));
    if (rc) return rc;
    for (int64_t i = 0; i < r.n_candidates; ++i) {
        const uint64_t key = P->cand_pos[static_cast<size_t>(i)] >= 0 ? P->h_cand_keys[P->cand_pos[static_cast<size_t>(i)]] : 0ull;
        if (key) mi355playlist::score_some(r, out, i, mi355rec_key_score(key));
        else mi355playlist::score_none(out, i);
    }
    return MI355REC_OK;
}

// The scoring entry points' shared tail: the list's and the call's own checks, then the one path.
int score_request(mi355rec* h, Request r, const int64_t* candidates, int64_t n_candidates, float* out_value, uint8_t* out_admissible) {
    char why[160];
    if (r.rowset && r.rowset->node) return fail(h, MI355REC_ERR_INVALID_ARG, "row set of another handle");
    if (mi355cand::invalid_count(candidates, n_candidates, MI355REC_MAX_CANDIDATES, why, sizeof why) ||
        mi355playlist::invalid_score_request(r, n_candidates, out_value, why, sizeof why))
        return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    if (mi355playlist::invalid_playlist(r, h->n, static_cast<int64_t>(UINT32_MAX) + 1, kMaxExclude, why, sizeof why))
        return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    if (n_candidates == 0) return MI355REC_OK;   // nothing to write, nothing to launch
    r.candidates_id_end = kRowsetIdEnd;   // (the ids are checked in playlist_launch's one pass over them)
    r.listed = r.score = true;
    r.candidates = candidates;
    r.n_candidates = n_candidates;
    return sync_playlist_scores(h, r, {out_value, out_admissible});
}

// The ONE body of every exported entry point that takes a request struct (playlist_request.h: from_request converts whichever it
// is): the null handle, the conversion, then the way down: score_request with `score` (its own checks), else the row set's owner,
// the list's count (candidates.h; the ids are checked in playlist_launch's one pass over them) and sync_playlist_query.
template <class Query, class Result>
int request_entry(mi355rec* h, const Query* query, const mi355rec_request_ext_t* ext, const Result* result,
                  const mi355playlist::CandidateList& list, const mi355playlist::ScoreOutputs* score = nullptr) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    Query full;
    Request r;
    Outputs out;
    char why[160];
    if (mi355playlist::from_request(query, ext, result, &full, &r, &out, why, sizeof why)) return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    if (score) return score_request(h, r, list.ids, list.n, score->value, score->admissible);
    if (r.rowset && r.rowset->node) return fail(h, MI355REC_ERR_INVALID_ARG, "row set of another handle");
    if (list.given) {
        if (mi355cand::invalid_count(list.ids, list.n, MI355REC_MAX_CANDIDATES, why, sizeof why))
            return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
        r.candidates_id_end = kRowsetIdEnd;
        r.listed = true;
        r.candidates = list.ids;
        r.n_candidates = list.n;
    }
    return sync_playlist_query(h, r, out);
}

}  // namespace

namespace mi355node {
int query_playlist(mi355rec_t* h, const mi355playlist::Request& r, const mi355playlist::Outputs& out) {
    return sync_playlist_query(h, r, out, kPlExcludeCap);
}
int score_playlist(mi355rec_t* h, const mi355playlist::Request& r, const mi355playlist::ScoreOutputs& out) {
    return sync_playlist_scores(h, r, out, kPlExcludeCap);
}
int set_group_priors(mi355rec_t* h, const float* priors_host, int64_t n) { return set_priors_common(h, priors_host, n, true); }
}  // namespace mi355node

extern "C" {

int mi355rec_query_mean_topn(mi355rec_t* h, const float* queries, int k, const int64_t* exclude_global, int n_exclude, int topn,
                             int64_t* out_idx, float* out_score, int* out_count) {
    return sync_playlist_query(h, request(queries, nullptr, nullptr, k, exclude_global, n_exclude, nullptr, topn),
                               {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_query_playlist_topn(mi355rec_t* h, const int64_t* local_rows, int k, const int64_t* exclude_global, int n_exclude,
                                 int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sync_playlist_query(h, request(nullptr, local_rows, nullptr, k, exclude_global, n_exclude, nullptr, topn),
                               {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_query_mean_topn_where(mi355rec_t* h, const float* queries, int k, const int64_t* exclude_global, int n_exclude,
                                   const mi355rec_filter_t* filter, int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sync_playlist_query(h, request(queries, nullptr, nullptr, k, exclude_global, n_exclude, filter, topn),
                               {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_query_playlist_topn_where(mi355rec_t* h, const int64_t* local_rows, int k, const int64_t* exclude_global,
                                       int n_exclude, const mi355rec_filter_t* filter, int topn, int64_t* out_idx, float* out_score,
                                       int* out_count) {
    return sync_playlist_query(h, request(nullptr, local_rows, nullptr, k, exclude_global, n_exclude, filter, topn),
                               {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_query_mean_topn_weighted(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                      int n_exclude, const mi355rec_filter_t* filter, int topn, int64_t* out_idx, float* out_score,
                                      int* out_count) {
    return sync_playlist_query(h, request(queries, nullptr, weights, k, exclude_global, n_exclude, filter, topn),
                               {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_query_playlist_topn_weighted(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                          const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, int topn,
                                          int64_t* out_idx, float* out_score, int* out_count) {
    return sync_playlist_query(h, request(nullptr, local_rows, weights, k, exclude_global, n_exclude, filter, topn),
                               {out_idx, out_score, nullptr, out_count, nullptr});
}

// "PLAYLIST REQUESTS": the family's one call; every entry point above (and engine_diverse.hip.h's) is a special case of it.
// "ROW SETS": the request with its per-request extras; the plain and the _scaled entry points are special cases of THIS one path.
// Every export from here to mi355rec_set_priors is request_entry (above) with its own structs.
int mi355rec_query_playlist_request_ext(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_request_ext_t* ext,
                                        const mi355rec_playlist_result_t* result) {
    return request_entry(h, query, ext, result, {});
}

// "CANDIDATE LISTS": the same request with its list; every check of the _ext call first, then the list's own (candidates.h).
int mi355rec_query_playlist_request_candidates(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, const mi355rec_playlist_result_t* result) {
    return request_entry(h, query, ext, result, {true, candidates, n_candidates});
}

int mi355rec_query_playlist_request_scaled(mi355rec_t* h, const mi355rec_playlist_query_t* query, const float* feature_scales,
                                           const mi355rec_playlist_result_t* result) {
    const mi355rec_request_ext_t ext = mi355playlist::scales_only_ext(feature_scales);
    return mi355rec_query_playlist_request_ext(h, query, &ext, result);
}

int mi355rec_query_playlist_request(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_playlist_result_t* result) {
    return mi355rec_query_playlist_request_ext(h, query, nullptr, result);
}

// "DISTANCE REQUESTS": the same Request with metric = kDistance through the same path.
int mi355rec_query_distance_request_ext(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_request_ext_t* ext,
                                        const mi355rec_distance_result_t* result) {
    return request_entry(h, query, ext, result, {});
}

int mi355rec_query_distance_request_candidates(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, const mi355rec_distance_result_t* result) {
    return request_entry(h, query, ext, result, {true, candidates, n_candidates});
}

// "CANDIDATE SCORES": the _candidates calls' conversion (there is no result struct: an empty one stands in), then score_request.
int mi355rec_score_playlist_request_candidates(mi355rec_t* h, const mi355rec_playlist_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, float* out_value, uint8_t* out_admissible) {
    const mi355rec_playlist_result_t none = {};
    const mi355playlist::ScoreOutputs score = {out_value, out_admissible};
    return request_entry(h, query, ext, &none, {true, candidates, n_candidates}, &score);
}

int mi355rec_score_distance_request_candidates(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_request_ext_t* ext,
                                               const int64_t* candidates, int64_t n_candidates, float* out_distance, uint8_t* out_admissible) {
    const mi355rec_distance_result_t none = {};
    const mi355playlist::ScoreOutputs score = {out_distance, out_admissible};
    return request_entry(h, query, ext, &none, {true, candidates, n_candidates}, &score);
}

int mi355rec_query_distance_request_scaled(mi355rec_t* h, const mi355rec_distance_query_t* query, const float* feature_scales,
                                           const mi355rec_distance_result_t* result) {
    const mi355rec_request_ext_t ext = mi355playlist::scales_only_ext(feature_scales);
    return mi355rec_query_distance_request_ext(h, query, &ext, result);
}

int mi355rec_query_distance_request(mi355rec_t* h, const mi355rec_distance_query_t* query, const mi355rec_distance_result_t* result) {
    return mi355rec_query_distance_request_ext(h, query, nullptr, result);
}

// "ANY-OF REQUESTS": the same Request with metric = kAnyOf through the same path; its scan is anyof_scan_kernel.
int mi355rec_query_anyof_request(mi355rec_t* h, const mi355rec_anyof_query_t* query, const mi355rec_request_ext_t* ext,
                                 const mi355rec_anyof_result_t* result) {
    return request_entry(h, query, ext, result, {});
}

// "MANHATTAN REQUESTS": the same Request with metric = kManhattan through the same path; its scan is manhattan_scan_kernel.
int mi355rec_query_manhattan_request(mi355rec_t* h, const mi355rec_manhattan_query_t* query, const mi355rec_request_ext_t* ext,
                                     const mi355rec_manhattan_result_t* result) {
    return request_entry(h, query, ext, result, {});
}

// "JACCARD REQUESTS": the same Request with metric = kJaccard through the same path; its scan is playlist_scan_kernel's kPlJaccard
// branch, with no replica (no pre-filter: every row takes the chains).
int mi355rec_query_jaccard_request(mi355rec_t* h, const mi355rec_jaccard_query_t* query, const mi355rec_request_ext_t* ext,
                                   const mi355rec_jaccard_result_t* result) {
    return request_entry(h, query, ext, result, {});
}

// "BOUNDED REQUESTS": the same Request with `bounded` through the same path: the count launch, then the top-N launch where topn > 0.
int mi355rec_query_bounded_request(mi355rec_t* h, const mi355rec_bounded_query_t* query, const mi355rec_request_ext_t* ext,
                                   const mi355rec_bounded_result_t* result) {
    return request_entry(h, query, ext, result, {});
}

// "ROW PRIORS"
int mi355rec_set_priors(mi355rec_t* h, const float* priors_host, int64_t n) { return set_priors_common(h, priors_host, n, false); }

}  // extern "C"

// mi355rec_rebuild_replica (mi355rec.hip): the norms are a snapshot of the rows too; the next distance request builds them again.
// (The caller has drained the handle's stream.)
static void drop_distance_norms(mi355rec* h) {
    if (!h->playlist || !h->playlist->d_norms) return;
    (void)hipFree(h->playlist->d_norms);
    h->playlist->d_norms = nullptr;
    h->playlist->norms_built = false;
}

extern "C" {

int mi355rec_playlist_counters(const mi355rec_t* h, int64_t* queries, int64_t* rows_exact) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (queries) *queries = h->playlist_queries;
    if (rows_exact) {
        unsigned long long v = 0;
        if (h->playlist) {
            DeviceGuard guard(h->device);
            // (the calls are synchronous: the counter is settled; a blocking copy orders after them anyway)
            const hipError_t e = hipMemcpy(&v, h->playlist->d_exact, sizeof v, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail(const_cast<mi355rec_t*>(h), MI355REC_ERR_HIP, "reading the playlist counter: %s", hipGetErrorString(e));
        }
        *rows_exact = static_cast<int64_t>(v);
    }
    return MI355REC_OK;
}

// "CANDIDATE LISTS": requests that took the gather launch, and the distinct in-shard list entries those launches were given.
int mi355rec_candidates_counters(const mi355rec_t* h, int64_t* requests, int64_t* rows_gathered) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (requests) *requests = h->playlist ? h->playlist->cand_requests : 0;
    if (rows_gathered) *rows_gathered = h->playlist ? h->playlist->cand_rows : 0;
    return MI355REC_OK;
}

}  // extern "C"
