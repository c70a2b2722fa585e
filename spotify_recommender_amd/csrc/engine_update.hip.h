// engine_update.hip.h — ROW UPDATES on the single-device handle (include/mi355rec_diag.h, "ROW UPDATES"): mi355rec_update_rows
// rewrites rows of the catalogue in place and redoes, for those rows only, everything the handle derives from a row alone —
// its entries in the fp16 and the 8-bit replica, its norm (distance requests) and its slot in the label-grouped copy — so
// that every route answers as a handle freshly made from the updated matrix would.  The device work is the UPDATE job of
// q8_build_kernel (replica_q8.hip.h): the packers it calls are the ones the builders call.  The snapshots that are only ever
// used to place a bound (the anchor table, the bucketed sample) may stay stale: the caller's anchor table is recopied because
// that is cheap, the rest waits for mi355rec_rebuild_replica (mi355rec_update_info_t::rows_since_snapshot is the cue).
// The checks of a list of rows are host-only code in rows_update.h.
// (Part of mi355rec.hip's translation unit, included last.)
#pragma once

#include <chrono>

#include "engine_labels.hip.h"
#include "engine_playlist.hip.h"
#include "rows_update.h"

namespace {

bool owns_matrix(const mi355rec* h) { return h->owned_feats || (h->shared && h->shared->owned_feats); }

// A streamed query or batch that has been accepted and not completed: its sample or cutoff was taken from the rows as they were.
bool stream_open(const mi355rec* m) { return m->stashed.has || m->pending || pairs_open(m) || m->mstash.has || m->mpending.has; }

// The staging of one chunk of `rows` rows (<= mi355update::kStageRows): [ids][sorted positions][rows x 12 floats], packed, in
// pinned memory and on the device.  The handle's stream is idle when this is called (every chunk waits for its launch).
int ensure_update_stage(mi355rec* h, int64_t rows) {
    mi355rec::Update& u = h->upd;
    if (rows <= u.cap) return MI355REC_OK;
    int64_t cap = u.cap ? u.cap : 256;
    while (cap < rows) cap *= 2;
    if (u.h_stage) (void)hipHostFree(u.h_stage);
    if (u.d_stage) (void)hipFree(u.d_stage);
    u.h_stage = u.d_stage = nullptr;
    u.cap = 0;
    const size_t bytes = static_cast<size_t>(cap) * (2 * sizeof(int64_t) + sizeof(float) * kDim);
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&u.h_stage), bytes, hipHostMallocDefault));
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&u.d_stage), bytes));
    u.cap = cap;
    return MI355REC_OK;
}

// The inverse of the label copy's d_rows, on the host, once per set of labels.
int ensure_label_positions(mi355rec* h, mi355rec_labels* L) {
    const size_t n = static_cast<size_t>(h->n);
    if (L->pos_of_row.size() == n) return MI355REC_OK;
    try {
        std::vector<uint32_t> order(n);
        HIP_TRY(h, hipMemcpy(order.data(), L->d_rows, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        L->pos_of_row.assign(n, 0u);
        for (size_t p = 0; p < n; ++p) L->pos_of_row[order[p]] = static_cast<uint32_t>(p);
    } catch (const std::bad_alloc&) {
        L->pos_of_row.clear();
        return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for the label positions (%lld rows)", (long long)h->n);
    }
    return MI355REC_OK;
}

int update_rows(mi355rec* h, const int64_t* local_rows, int64_t count, const float* feats_host) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (count < 0 || (count > 0 && !local_rows)) return fail(h, MI355REC_ERR_INVALID_ARG, "null rows / negative count");
    if (feats_host && !owns_matrix(h))
        return fail(h, MI355REC_ERR_INVALID_ARG, "this handle borrows its matrix (mi355rec_create_device): write the rows there and pass NULL");
    if (count == 0) return MI355REC_OK;
    try {
        int64_t at = 0;
        const mi355update::Bad bad = mi355update::check_rows(local_rows, count, h->n, &at);
        if (bad != mi355update::kFine) {
            char why[160];
            mi355update::describe(bad, local_rows, at, h->n, why, sizeof why);
            return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
        }
    } catch (const std::bad_alloc&) {
        return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory checking an update of %lld rows", (long long)count);
    }
    if (h->shared)
        for (const mi355rec* m : h->shared->members)
            if (m != h && stream_open(m))
                return fail(h, MI355REC_ERR_INVALID_ARG, "another lane of the group has a streamed query or batch open: flush every lane (mi355rec_enqueue_flush) before an update");
    DeviceGuard guard(h->device);
    const auto t0 = std::chrono::steady_clock::now();
    int rc = sync_api_begin(h);
    if (rc) return rc;
    // The rows and the replicas are written in place: nothing any OTHER member has enqueued may still be reading them.  A member's
    // flush only enqueues (its flags above are clear while its scans are in flight), so the call waits here, before the first
    // write, for every other member's own stream and for the stream it was last used on.  (sync_api_begin has ordered the
    // caller's own work; the call is synchronous, so a host wait costs nothing it would not pay anyway.)
    if (h->shared)
        for (mi355rec* m : h->shared->members) {
            if (m == h) continue;
            if (m->has_last_stream && m->last_stream != m->stream && hipStreamSynchronize(m->last_stream) != hipSuccess)
                (void)hipGetLastError();   // (a caller's stream that no longer exists: nothing left on it, as in order_stream)
            HIP_TRY(h, hipStreamSynchronize(m->stream));
        }
    rc = flush_streamed(h, h->stream);   // (as mi355rec_rebuild_replica: the handle's own stashed and pending queries see the old rows)
    if (rc) return rc;
    rc = flush_mstream(h, h->stream);
    if (rc) return rc;
    mi355rec_labels* L = h->side->labels;
    if (L && h->n > 0) {
        rc = ensure_label_positions(h, L);
        if (rc) return rc;
    }
    float* norms = h->playlist && h->playlist->norms_built ? h->playlist->d_norms : nullptr;
    float* matrix = const_cast<float*>(h->d_feats);   // (written only where the library owns it)
    const bool derived = h->d_half || h->d_q8 || norms;
    rc = ensure_update_stage(h, count < mi355update::kStageRows ? count : mi355update::kStageRows);
    if (rc) return rc;
    for (int64_t c0 = 0; c0 < count; c0 += mi355update::kStageRows) {
        const int64_t cnt = count - c0 < mi355update::kStageRows ? count - c0 : mi355update::kStageRows;
        // [ids][positions][rows], packed for this chunk: one copy
        int64_t* h_ids = reinterpret_cast<int64_t*>(h->upd.h_stage);
        int64_t* h_pos = h_ids + cnt;
        std::memcpy(h_ids, local_rows + c0, sizeof(int64_t) * static_cast<size_t>(cnt));
        for (int64_t i = 0; i < cnt; ++i) h_pos[i] = L ? static_cast<int64_t>(L->pos_of_row[static_cast<size_t>(h_ids[i])]) : 0;
        size_t bytes = sizeof(int64_t) * 2 * static_cast<size_t>(cnt);
        if (feats_host) {
            std::memcpy(h->upd.h_stage + bytes, feats_host + static_cast<size_t>(c0) * kDim, sizeof(float) * kDim * static_cast<size_t>(cnt));
            bytes += sizeof(float) * kDim * static_cast<size_t>(cnt);
        }
        HIP_TRY(h, hipMemcpyAsync(h->upd.d_stage, h->upd.h_stage, bytes, hipMemcpyHostToDevice, h->stream));
        const int64_t* d_ids = reinterpret_cast<const int64_t*>(h->upd.d_stage);
        const int64_t* d_pos = d_ids + cnt;
        const float* d_rows = reinterpret_cast<const float*>(d_pos + cnt);   // (16-byte aligned: 16 B of ids and positions per row before it)
        const dim3 grid(static_cast<unsigned>((cnt + 255) / 256));
        if (feats_host) {   // thread e: staged row e -> the matrix and every entry derived from it, at row ids[e]
            hipLaunchKernelGGL(q8_build_kernel, grid, dim3(256), 0, h->stream, d_rows, cnt, cnt, reinterpret_cast<uint32_t*>(h->d_q8), norms,
                               static_cast<const int32_t*>(nullptr), static_cast<const float*>(nullptr), 0, static_cast<int32_t*>(nullptr),
                               static_cast<const int64_t*>(nullptr), d_ids, reinterpret_cast<uint2*>(h->d_half), matrix);
        } else if (derived) {   // the caller has written the rows: thread e redoes what is derived from row ids[e] of the matrix
            hipLaunchKernelGGL(q8_build_kernel, grid, dim3(256), 0, h->stream, h->d_feats, h->n, cnt, reinterpret_cast<uint32_t*>(h->d_q8), norms,
                               static_cast<const int32_t*>(nullptr), static_cast<const float*>(nullptr), 0, static_cast<int32_t*>(nullptr),
                               d_ids, d_ids, reinterpret_cast<uint2*>(h->d_half), static_cast<float*>(nullptr));
        }
        if (L) {   // the label-grouped copy: the same job with the fp32 destination only, row ids[e] of the matrix -> its sorted position
            hipLaunchKernelGGL(q8_build_kernel, grid, dim3(256), 0, h->stream, h->d_feats, h->n, cnt, static_cast<uint32_t*>(nullptr),
                               static_cast<float*>(nullptr), static_cast<const int32_t*>(nullptr), static_cast<const float*>(nullptr), 0,
                               static_cast<int32_t*>(nullptr), d_ids, d_pos, static_cast<uint2*>(nullptr), L->d_feats);
        }
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the staging is free for the next chunk; the call is synchronous anyway)
    }
    // The norms belong to each handle: the caller's were rewritten above, the other members' are dropped and built again by
    // their next distance request.  (Every member's stream was drained above, and no other thread uses the group during the call.)
    if (h->shared)
        for (mi355rec* m : h->shared->members)
            if (m != h) {
                drop_distance_norms(m);
                m->upd.rows_since_snapshot += count;
            }
    // (4096 rows: cheap; the other members' tables stay, a stale one only picks a poorer centre.  If the recopy fails the rows
    // HAVE been updated and the counters say so: the error is reported, and repeating the call is safe.)
    rc = build_anchors(h);
    h->upd.calls += 1;
    h->upd.rows += count;
    h->upd.rows_since_snapshot += count;
    h->upd.last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// The bytes of `count` rows' entries of one per-row array (stride bytes per row) to the host, in the order asked: one copy per
// run of consecutive rows.
int copy_entries(mi355rec* h, const void* dev, size_t stride, const int64_t* rows, int64_t count, void* out) {
    for (int64_t i = 0; i < count;) {
        int64_t j = i + 1;
        while (j < count && rows[j] == rows[j - 1] + 1) ++j;
        HIP_TRY(h, hipMemcpy(static_cast<char*>(out) + static_cast<size_t>(i) * stride,
                             static_cast<const char*>(dev) + static_cast<size_t>(rows[i]) * stride, static_cast<size_t>(j - i) * stride,
                             hipMemcpyDeviceToHost));
        i = j;
    }
    return MI355REC_OK;
}

}  // namespace

extern "C" {

int mi355rec_update_rows(mi355rec_t* h, const int64_t* local_rows, int64_t count, const float* feats_host) {
    return update_rows(h, local_rows, count, feats_host);
}

int mi355rec_update_info(const mi355rec_t* h, mi355rec_update_info_t* out) {
    if (!h || !out) return fail(const_cast<mi355rec_t*>(h), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size < 2 * sizeof(uint32_t))
        return fail(const_cast<mi355rec_t*>(h), MI355REC_ERR_INVALID_ARG, "mi355rec_update_info_t::size %u: set it to sizeof of the struct", out->size);
    mi355rec_update_info_t full;
    std::memset(&full, 0, sizeof full);
    full.size = out->size < sizeof full ? out->size : static_cast<uint32_t>(sizeof full);
    full.last_ms = h->upd.last_ms;
    full.calls = h->upd.calls;
    full.rows = h->upd.rows;
    full.rows_since_snapshot = h->upd.rows_since_snapshot;
    std::memcpy(out, &full, full.size);   // (a caller built against a shorter header gets the fields it knows)
    return MI355REC_OK;
}

int mi355rec_replica_entries(mi355rec_t* h, const int64_t* local_rows, int64_t count, void* out_half, void* out_q8, float* out_norms) {
    if (!h) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (count < 0 || (count > 0 && !local_rows)) return fail(h, MI355REC_ERR_INVALID_ARG, "null rows / negative count");
    if (!h->d_half || !h->d_q8) return fail(h, MI355REC_ERR_INVALID_ARG, "this handle has no replicas (mi355rec_set_replica)");
    for (int64_t i = 0; i < count; ++i)
        if (local_rows[i] < 0 || local_rows[i] >= h->n)
            return fail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)local_rows[i]);
    DeviceGuard guard(h->device);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = MI355REC_OK;
    if (out_half) rc = copy_entries(h, h->d_half, 24, local_rows, count, out_half);
    if (!rc && out_q8) rc = copy_entries(h, h->d_q8, 12, local_rows, count, out_q8);
    if (!rc && out_norms && h->playlist && h->playlist->norms_built)
        rc = copy_entries(h, h->playlist->d_norms, sizeof(float), local_rows, count, out_norms);
    return rc;
}

}  // extern "C"
