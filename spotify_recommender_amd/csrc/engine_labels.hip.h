// engine_labels.hip.h — LABELS on the single-device handle (include/mi355rec_diag.h, "LABELS"): the label-grouped copy of
// the shard's rows that mi355rec_set_labels builds (and the labels in row order for the playlist calls), and the synchronous
// filtered query over it (labels.hip.h, then the merge of merge.hip.h, between sync_begin and sync_finish of
// engine_sync.hip.h).  Also the owner's side of the PER-ROW SIDE DATA (RowSide, engine_state.hip.h): free_side, and
// replace_side, which the setters of labels, groups and priors share.
// (Part of mi355rec.hip's translation unit, included after engine_sync.hip.h.)
#pragma once

#include <chrono>

#include "engine_sync.hip.h"
#include "labels.hip.h"
#include "playlist_request.h"

// What mi355rec_set_labels leaves on the device, and the offsets again on the host (they size a query's grid).
struct mi355rec_labels {
    float* d_feats = nullptr;     // [n][12]: the rows, grouped by label (ascending), stable inside a label, unlabelled last
    uint32_t* d_rows = nullptr;   // [n]: the shard-local row of each sorted position
    int64_t* d_off = nullptr;     // [kMaxLabels + 1]: label l holds positions [d_off[l], d_off[l + 1])
    int16_t* d_row_labels = nullptr;   // [ceil(n / 4) * 4]: the labels in ROW order, the last quad padded with -1 (what a playlist
                                       // call with a label set reads, playlist.hip.h "LABEL SET": 2 B per row)
    std::vector<int64_t> off;     // the same offsets on the host
    std::vector<uint32_t> pos_of_row;   // the inverse of d_rows, on the host: made by the first mi355rec_update_rows (engine_update.hip.h)
    int grid_cap = 1;             // workgroups of a filtered launch at most (occupancy x CUs, and the handle's list slots)
    float build_ms = 0.0f;        // wall time of the mi355rec_set_labels call that built it
};

namespace {

void free_labels(mi355rec_labels* L) {
    if (!L) return;
    void* bufs[] = {L->d_feats, L->d_rows, L->d_off, L->d_row_labels};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete L;
}

// Frees what a RowSide holds and leaves it empty: the one place the side data is freed.
void free_side(RowSide& s) {
    free_labels(s.labels);
    if (s.d_groups) (void)hipFree(s.d_groups);
    if (s.d_priors) (void)hipFree(s.d_priors);
    s = RowSide();
}

// What the three setters share: `field` of the side data `h` answers from is replaced by what `build` makes (`set`), or
// dropped (!set).  A handle with lanes refuses, unless `group_ok`: the side data may be replaced under a group of lanes only
// for a caller that knows no member of the group is in use meanwhile (the node handle, whose workers are idle and whose
// replicas on one device are lanes of the first).  build(&fresh) validates and uploads; where it fails the previous value
// stays.  The old value is freed once the handle's stream has drained (only the synchronous calls on it read side data).
template <class T, class Build>
int replace_side(mi355rec* h, T* RowSide::*field, const char* noun, bool group_ok, bool set, Build build) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (!group_ok && h->shared && (h->is_lane || h->shared->refs.load() > 1))
        return fail(h, MI355REC_ERR_INVALID_ARG, "the handle has lanes: set the %s before the first lane is made", noun);
    DeviceGuard guard(h->device);
    T* fresh = nullptr;
    if (set) {
        const int rc = build(&fresh);
        if (rc != MI355REC_OK) {
            (void)hipGetLastError();   // (a failed upload leaves no HIP error behind)
            return rc;
        }
    }
    RowSide old;
    old.*field = h->side->*field;
    if (old.*field) (void)hipStreamSynchronize(h->stream);
    free_side(old);
    h->side->*field = fresh;
    return MI355REC_OK;
}

// Builds the label-grouped copy: the rows come back to the host (the handle may have been made from a device pointer),
// are placed by a counting sort and go up again.  Nothing of the handle is touched until everything has succeeded.
int build_labels(mi355rec* h, const int32_t* labels, mi355rec_labels** out) {
    *out = nullptr;
    const size_t n = static_cast<size_t>(h->n);
    mi355rec_labels* L = new (std::nothrow) mi355rec_labels();
    if (!L) return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for the labels");
    std::vector<float> rows, sorted;
    std::vector<uint32_t> order;
    std::vector<int16_t> in_row_order;
    const size_t n_padded = (n + 3) / 4 * 4;
    try {   // (no exception may cross the C-ABI)
        L->off.assign(kMaxLabels + 2, 0);
        rows.resize(n * kDim);
        sorted.resize(n * kDim);
        order.resize(n);
        in_row_order.assign(n_padded, static_cast<int16_t>(-1));
    } catch (const std::bad_alloc&) {
        free_labels(L);
        return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for the labels (%lld rows)", (long long)h->n);
    }
    // counting sort: bucket l for label l, bucket kMaxLabels for the unlabelled rows
    std::vector<int64_t>& off = L->off;
    for (size_t i = 0; i < n; ++i) ++off[(labels[i] < 0 ? kMaxLabels : labels[i]) + 1];
    for (int l = 0; l <= kMaxLabels; ++l) off[l + 1] += off[l];
    {
        std::vector<int64_t> next(off.begin(), off.end() - 1);
        for (size_t i = 0; i < n; ++i) order[next[labels[i] < 0 ? kMaxLabels : labels[i]]++] = static_cast<uint32_t>(i);
    }
    off.resize(kMaxLabels + 1);   // (the end of the unlabelled bucket is n)
    for (size_t i = 0; i < n; ++i) in_row_order[i] = static_cast<int16_t>(labels[i] < 0 ? -1 : labels[i]);   // (kMaxLabels fits int16)
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, label_scan_kernel, LabelScanCfg::kBlock, 0) != hipSuccess || occ < 1) occ = 1;
    (void)hipGetLastError();
    L->grid_cap = h->cus * occ;
    if (L->grid_cap > h->geom[kFp32].grid) L->grid_cap = h->geom[kFp32].grid;   // d_block_lists holds at least that many lists of kMaxTopK keys
    if (L->grid_cap < 1) L->grid_cap = 1;
    auto failed = [&](hipError_t e, const char* what) {
        free_labels(L);
        return fail(h, e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    };
    hipError_t e = hipMalloc(&L->d_off, sizeof(int64_t) * (kMaxLabels + 1));
    if (e != hipSuccess) return failed(e, "hipMalloc(label offsets)");
    if (n > 0) {
        if ((e = hipMalloc(&L->d_feats, sizeof(float) * kDim * n)) != hipSuccess) return failed(e, "hipMalloc(label-grouped rows)");
        if ((e = hipMalloc(&L->d_rows, sizeof(uint32_t) * n)) != hipSuccess) return failed(e, "hipMalloc(label row ids)");
        // (on the handle's stream, behind whatever the handle has enqueued there: a caller's kernel that wrote a borrowed
        // matrix is the caller's to have finished, as for create)
        if ((e = hipMemcpyAsync(rows.data(), h->d_feats, sizeof(float) * kDim * n, hipMemcpyDeviceToHost, h->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(h->stream)) != hipSuccess)
            return failed(e, "gathering the rows (D2H)");
        for (size_t p = 0; p < n; ++p) std::memcpy(&sorted[p * kDim], &rows[static_cast<size_t>(order[p]) * kDim], sizeof(float) * kDim);
        if ((e = hipMemcpy(L->d_feats, sorted.data(), sizeof(float) * kDim * n, hipMemcpyHostToDevice)) != hipSuccess)
            return failed(e, "hipMemcpy(label-grouped rows H2D)");
        if ((e = hipMemcpy(L->d_rows, order.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) != hipSuccess)
            return failed(e, "hipMemcpy(label row ids H2D)");
        if ((e = hipMalloc(&L->d_row_labels, sizeof(int16_t) * n_padded)) != hipSuccess) return failed(e, "hipMalloc(labels in row order)");
        if ((e = hipMemcpy(L->d_row_labels, in_row_order.data(), sizeof(int16_t) * n_padded, hipMemcpyHostToDevice)) != hipSuccess)
            return failed(e, "hipMemcpy(labels in row order H2D)");
    }
    if ((e = hipMemcpy(L->d_off, off.data(), sizeof(int64_t) * (kMaxLabels + 1), hipMemcpyHostToDevice)) != hipSuccess)
        return failed(e, "hipMemcpy(label offsets H2D)");
    *out = L;
    return MI355REC_OK;
}

// The query's label set as a mask; *rows = the selected rows, *tiles = the tiles of 512 rows they make (per label).
int label_mask(mi355rec* h, const mi355rec_labels* L, const int32_t* labels, int n_labels, LabelMask* mask, int64_t* rows,
               int64_t* tiles) {
    if (n_labels <= 0) return fail(h, MI355REC_ERR_INVALID_ARG, "n_labels must be positive, got %d", n_labels);
    if (!labels) return fail(h, MI355REC_ERR_INVALID_ARG, "null label set");
    std::memset(mask, 0, sizeof *mask);
    for (int i = 0; i < n_labels; ++i) {
        const int32_t l = labels[i];
        if (l < 0 || l >= kMaxLabels)
            return fail(h, MI355REC_ERR_INVALID_ARG, "label %d out of [0, %d)", static_cast<int>(l), kMaxLabels);
        mask->w[l >> 5] |= 1u << (l & 31);
    }
    *rows = 0;
    *tiles = 0;
    for (int l = 0; l < kMaxLabels; ++l) {
        if (!((mask->w[l >> 5] >> (l & 31)) & 1u)) continue;
        const int64_t c = L->off[l + 1] - L->off[l];
        *rows += c;
        *tiles += (c + LabelScanCfg::kTileRows - 1) / LabelScanCfg::kTileRows;
    }
    return MI355REC_OK;
}

// One filtered query, synchronously (engine_sync.hip.h): rounds of kMaxTopK keys, each one label_scan_kernel launch + one
// merge; a single-round query's merge stores the results and the completion word in pinned host memory.
int sync_label_query(mi355rec* h, const float* qptr, const float* query12, int64_t exclude_global, const int32_t* labels,
                     int n_labels, int topn, int64_t* out_idx, float* out_score, int* out_count) {
    int rc = check_topn(h, topn, true);
    if (rc) return rc;
    const mi355rec_labels* L = h->side->labels;
    if (!L) return fail(h, MI355REC_ERR_INVALID_ARG, "this handle has no labels (mi355rec_set_labels)");
    LabelMask mask;
    int64_t selected = 0, tiles = 0;
    rc = label_mask(h, L, labels, n_labels, &mask, &selected, &tiles);
    if (rc) return rc;
    ++h->label_queries;
    const int eff = static_cast<int64_t>(topn) < selected ? topn : static_cast<int>(selected);
    if (eff == 0) {   // nothing selected: nothing to launch
        mi355playlist::pad({out_idx, out_score, nullptr, out_count, nullptr}, 0, topn, 0);
        return MI355REC_OK;
    }
    DeviceGuard guard(h->device);
    SyncSlots ss;
    rc = sync_begin(h, eff, 1, true, &ss);
    if (rc) return rc;
    QueryArg qa;
    std::memset(&qa, 0, sizeof qa);
    if (!qptr) std::memcpy(qa.q, query12, sizeof qa.q);
    const int grid = static_cast<int>(tiles < L->grid_cap ? tiles : L->grid_cap);
    for (int done = 0; done < eff; done += kMaxTopK) {
        const int k = eff - done < kMaxTopK ? eff - done : kMaxTopK;
        const uint64_t* upper = done ? h->d_keys + done - 1 : nullptr;
        LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, label_scan_kernel, dim3(grid), dim3(LabelScanCfg::kBlock),
                     h->stream, L->d_feats, L->d_rows, L->d_off, mask, h->row_base, qa, qptr, exclude_global, k,
                     h->d_block_lists, upper);
        HIP_TRY(h, hipGetLastError());
        h->label_rows_scanned += tiles * LabelScanCfg::kTileRows;
        rc = enqueue_merge(h, h->d_block_lists, grid, k, k, h->d_keys + done, ss.idx + done, ss.score + done, h->stream, ss.want);
        if (rc) return rc;
    }
    return sync_finish(h, ss, topn, out_idx, out_score, out_count);
}

// mi355rec_set_labels: the labels' own checks and build (replace_side does the rest).
int set_labels_common(mi355rec* h, const int32_t* labels_host, int64_t n, bool group_ok) {
    return replace_side(h, &RowSide::labels, "labels", group_ok, labels_host != nullptr, [&](mi355rec_labels** fresh) {
        if (n != h->n) return fail(h, MI355REC_ERR_INVALID_ARG, "%lld labels for a handle of %lld rows", (long long)n, (long long)h->n);
        for (int64_t i = 0; i < n; ++i)
            if (labels_host[i] < -1 || labels_host[i] >= kMaxLabels)
                return fail(h, MI355REC_ERR_INVALID_ARG, "label %d of row %lld out of [-1, %d)", static_cast<int>(labels_host[i]),
                            (long long)i, kMaxLabels);
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = build_labels(h, labels_host, fresh);
        if (rc == MI355REC_OK)
            (*fresh)->build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    });
}

}  // namespace

namespace mi355node {
int set_group_labels(mi355rec_t* h, const int32_t* labels_host, int64_t n) { return set_labels_common(h, labels_host, n, true); }
}  // namespace mi355node

extern "C" {

int mi355rec_set_labels(mi355rec_t* h, const int32_t* labels_host, int64_t n) {
    return set_labels_common(h, labels_host, n, false);
}

int mi355rec_query_row_topn_labels(mi355rec_t* h, int64_t local_row, const int32_t* labels, int n_labels, int topn,
                                   int64_t* out_idx, float* out_score, int* out_count) {
    if (!h || !out_idx) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (local_row < 0 || local_row >= h->n)
        return fail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)local_row);
    return sync_label_query(h, h->d_feats + local_row * kDim, nullptr, h->row_base + local_row, labels, n_labels, topn, out_idx,
                            out_score, out_count);
}

int mi355rec_query_topn_labels(mi355rec_t* h, const float* query12, int64_t exclude_global, const int32_t* labels, int n_labels,
                               int topn, int64_t* out_idx, float* out_score, int* out_count) {
    if (!h || !query12 || !out_idx) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    return sync_label_query(h, nullptr, query12, exclude_global, labels, n_labels, topn, out_idx, out_score, out_count);
}

int mi355rec_label_counters(const mi355rec_t* h, int64_t* queries, int64_t* rows_scanned) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (queries) *queries = h->label_queries;
    if (rows_scanned) *rows_scanned = h->label_rows_scanned;
    return MI355REC_OK;
}

}  // extern "C"
