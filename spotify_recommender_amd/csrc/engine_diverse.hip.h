// engine_diverse.hip.h — DIVERSIFIED TOP-N on the single-device handle (include/mi355rec_diag.h, "DIVERSIFIED TOP-N"): the
// weighted playlist call's top-`pool`, re-ranked by maximal marginal relevance.  What sync_playlist_query
// (engine_playlist.hip.h) does for a diversified request: the scan launch of the playlist call, the merge into h->d_keys (no
// ids or scores are unpacked: the pool never leaves the device), then mmr_rerank_kernel (diverse.hip.h) on the same stream,
// which stores the picks into the handle's pinned result slots and raises the completion word: the host waits once
// (sync_finish, engine_sync.hip.h; the slots were begun by playlist_launch).  Here: that request's checks, the re-rank and
// its extra outputs (mmr, P'), mi355rec_set_groups, the _diverse and _capped entry points, a pool passed by value (what a
// row-sharded node does after gathering the pool's rows from its shards) and mi355rec_fetch_rows, both launches of the same
// kernel.  (Part of mi355rec.hip's translation unit, included after engine_playlist.hip.h.)
#pragma once

#include <cmath>

#include "diverse.hip.h"
#include "engine_playlist.hip.h"

namespace {

// lambda, topn, pool and the cap (the other arguments are the playlist call's, checked by playlist_launch with topn = pool).
int check_diverse(mi355rec* h, const Request& r) {
    char why[128];
    if (mi355playlist::invalid_diverse(r, why, sizeof why)) return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    if (r.capped && !h->side->d_groups) return fail(h, MI355REC_ERR_INVALID_ARG, "this handle has no groups (mi355rec_set_groups)");
    return MI355REC_OK;
}

// The pinned mmr slots and the device rows of the diversified calls (the playlist state holds them).
int ensure_diverse(mi355rec* h) {
    const int rc = ensure_playlist(h);
    if (rc) return rc;
    mi355rec_playlist* P = h->playlist;
    if (!P->h_mmr) {   // (one word more: P' of a capped call)
        HIP_TRY(h, hipHostMalloc(&P->h_mmr, sizeof(float) * kMaxTopK + sizeof(int), hipHostMallocMapped));
        HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&P->hd_mmr), P->h_mmr, 0));
        P->h_pool_rows = reinterpret_cast<int*>(P->h_mmr + kMaxTopK);
        P->hd_pool_rows = reinterpret_cast<int*>(P->hd_mmr + kMaxTopK);
    }
    if (!P->d_rows) HIP_TRY(h, hipMalloc(&P->d_rows, sizeof(float) * kDim * kMaxTopK));
    if (!P->d_pool_groups) HIP_TRY(h, hipMalloc(&P->d_pool_groups, sizeof(int32_t) * kMaxTopK));
    return MI355REC_OK;
}

// The re-rank of the `pool` keys in h->d_keys on h->stream, the wait and the results; of `r`: lambda, topn and the cap.
// Over the handle's matrix and (GROUP CAPS: the same launch, two more arguments) its groups, or — staged — over the pool's
// rows and groups in pool order, copied to the playlist state by the caller.  The kernel itself stores the picks into the
// pinned slots and raises ss.want; beyond sync_finish only the extra outputs (mmr, P') are this function's.
int rerank_and_wait(mi355rec* h, const Request& r, const Outputs& out, SyncSlots ss, int pool, bool staged) {
    mi355rec_playlist* P = h->playlist;
    const float* rows = staged ? P->d_rows : h->d_feats;
    const int32_t* groups = !r.capped ? nullptr : staged ? P->d_pool_groups : h->side->d_groups;
    const int topn = r.topn;
    const float mu = 1.0f - r.lambda;
    const int block = (pool + 63) & ~63;
    hipLaunchKernelGGL(mmr_rerank_kernel, dim3(1), dim3(block), 0, h->stream, static_cast<const uint64_t*>(h->d_keys), rows, h->n,
                       h->row_base, staged ? 1 : 0, pool, topn, r.lambda, mu, ss.idx, ss.score, P->hd_mmr,
                       static_cast<float*>(nullptr), h->hd_done, ss.want, groups, r.max_per_group,
                       groups ? P->hd_pool_rows : static_cast<int*>(nullptr));
    HIP_TRY(h, hipGetLastError());
    ss.eff = topn;   // (the slots were begun for the pool; its topn picks are the call's results)
    const int rc = sync_finish(h, ss, topn, out.idx, out.score, out.count);
    if (rc) return rc;
    if (out.pool_rows) *out.pool_rows = groups ? *P->h_pool_rows : 0;
    if (out.mmr) std::memcpy(out.mmr, P->h_mmr, static_cast<size_t>(topn) * sizeof(float));
    return MI355REC_OK;
}

// mi355rec_set_groups: the groups' own checks and upload (replace_side, engine_labels.hip.h, does the rest).
int set_groups_common(mi355rec* h, const int32_t* groups_host, int64_t n, bool group_ok) {
    return replace_side(h, &RowSide::d_groups, "groups", group_ok, groups_host != nullptr, [&](int32_t** fresh) {
        if (n != h->n) return fail(h, MI355REC_ERR_INVALID_ARG, "%lld groups for a handle of %lld rows", (long long)n, (long long)h->n);
        for (int64_t i = 0; i < n; ++i)
            if (groups_host[i] < -1)
                return fail(h, MI355REC_ERR_INVALID_ARG, "group %d of row %lld: a group id is >= 0, or -1 for no group",
                            static_cast<int>(groups_host[i]), (long long)i);
        // (an empty shard keeps a one-word array: "has groups" is a non-null pointer)
        hipError_t e = hipMalloc(fresh, sizeof(int32_t) * static_cast<size_t>(n > 0 ? n : 1));
        if (e == hipSuccess && n > 0) e = hipMemcpy(*fresh, groups_host, sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyHostToDevice);
        if (e == hipSuccess) return static_cast<int>(MI355REC_OK);
        if (*fresh) (void)hipFree(*fresh);
        return fail(h, e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, "the groups (%lld rows): %s",
                    (long long)n, hipGetErrorString(e));
    });
}

}  // namespace

namespace mi355node {
int set_group_groups(mi355rec_t* h, const int32_t* groups_host, int64_t n) { return set_groups_common(h, groups_host, n, true); }

int rerank_pool(mi355rec_t* h, const int64_t* pool_idx, const float* pool_score, const float* pool_rows, int count, float lambda, int topn,
                int64_t* out_idx, float* out_score, float* out_mmr, int* out_count, const int32_t* pool_groups, int max_per_group,
                int* out_pool_rows) {
    if (!h || !pool_idx || !pool_score || !pool_rows || !out_idx) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (count < 1 || count > kMaxTopK || topn < 1 || topn > kMaxTopK)
        return fail(h, MI355REC_ERR_INVALID_ARG, "a pool of %d rows, topn %d: 1 to %d are supported", count, topn, kMaxTopK);
    if (pool_groups && max_per_group < 1)
        return fail(h, MI355REC_ERR_INVALID_ARG, "max_per_group must be positive, got %d", max_per_group);
    DeviceGuard guard(h->device);
    SyncSlots ss;
    int rc = ensure_diverse(h);
    if (!rc) rc = sync_begin(h, kMaxTopK, 1, true, &ss);   // (slots for any pool and topn this call takes)
    if (rc) return rc;
    uint64_t keys[kMaxTopK];
    for (int i = 0; i < count; ++i) keys[i] = pack_key(pool_score[i], static_cast<uint32_t>(pool_idx[i]));
    // (pageable sources: each copy has left the host buffer when the call returns)
    HIP_TRY(h, hipMemcpyAsync(h->d_keys, keys, sizeof(uint64_t) * static_cast<size_t>(count), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->playlist->d_rows, pool_rows, sizeof(float) * kDim * static_cast<size_t>(count), hipMemcpyHostToDevice,
                              h->stream));
    if (pool_groups)
        HIP_TRY(h, hipMemcpyAsync(h->playlist->d_pool_groups, pool_groups, sizeof(int32_t) * static_cast<size_t>(count),
                                  hipMemcpyHostToDevice, h->stream));
    Request r;   // (what the re-rank reads of a request)
    r.lambda = lambda;
    r.topn = topn;
    r.capped = pool_groups != nullptr;
    r.max_per_group = max_per_group;
    return rerank_and_wait(h, r, {out_idx, out_score, out_mmr, out_count, out_pool_rows}, ss, count, true);
}
}  // namespace mi355node

extern "C" {

int mi355rec_query_mean_topn_diverse(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                     int n_exclude, const mi355rec_filter_t* filter, float lambda, int pool, int topn, int64_t* out_idx,
                                     float* out_score, float* out_mmr, int* out_count) {
    return sync_playlist_query(h, request(queries, nullptr, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool),
                               {out_idx, out_score, out_mmr, out_count, nullptr});
}

int mi355rec_query_playlist_topn_diverse(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                         const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, float lambda,
                                         int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr, int* out_count) {
    return sync_playlist_query(h, request(nullptr, local_rows, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool),
                               {out_idx, out_score, out_mmr, out_count, nullptr});
}

int mi355rec_set_groups(mi355rec_t* h, const int32_t* groups_host, int64_t n) { return set_groups_common(h, groups_host, n, false); }

int mi355rec_query_mean_topn_capped(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                    int n_exclude, const mi355rec_filter_t* filter, float lambda, int pool, int max_per_group, int topn,
                                    int64_t* out_idx, float* out_score, float* out_mmr, int* out_count, int* out_pool_rows) {
    return sync_playlist_query(
        h, request(queries, nullptr, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool).capped_at(max_per_group),
        {out_idx, out_score, out_mmr, out_count, out_pool_rows});
}

int mi355rec_query_playlist_topn_capped(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                        const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, float lambda,
                                        int pool, int max_per_group, int topn, int64_t* out_idx, float* out_score, float* out_mmr,
                                        int* out_count, int* out_pool_rows) {
    return sync_playlist_query(
        h, request(nullptr, local_rows, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool).capped_at(max_per_group),
        {out_idx, out_score, out_mmr, out_count, out_pool_rows});
}

int mi355rec_fetch_rows(mi355rec_t* h, const int64_t* local_rows, int64_t count, float* out_host) {
    if (!h || (count > 0 && (!local_rows || !out_host))) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (count < 0) return fail(h, MI355REC_ERR_INVALID_ARG, "count %lld is negative", (long long)count);
    for (int64_t i = 0; i < count; ++i)
        if (local_rows[i] < 0 || local_rows[i] >= h->n)
            return fail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)local_rows[i]);
    if (count == 0) return MI355REC_OK;
    DeviceGuard guard(h->device);
    SyncSlots ss;   // (only h->d_keys of the slots is used; never notifies: each round waits for the stream)
    int rc = ensure_diverse(h);
    if (!rc) rc = sync_begin(h, kMaxTopK, 1, false, &ss);
    if (rc) return rc;
    uint64_t keys[kMaxTopK];
    for (int64_t done = 0; done < count; done += kMaxTopK) {   // one gather launch and one copy back per 1024 rows
        const int c = static_cast<int>(count - done < kMaxTopK ? count - done : kMaxTopK);
        for (int i = 0; i < c; ++i) keys[i] = pack_key(0.0f, static_cast<uint32_t>(h->row_base + local_rows[done + i]));
        HIP_TRY(h, hipMemcpyAsync(h->d_keys, keys, sizeof(uint64_t) * static_cast<size_t>(c), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(mmr_rerank_kernel, dim3(1), dim3((c + 63) & ~63), 0, h->stream, static_cast<const uint64_t*>(h->d_keys),
                           static_cast<const float*>(h->d_feats), h->n, h->row_base, 0, c, 0, 0.0f, 0.0f, static_cast<int64_t*>(nullptr),
                           static_cast<float*>(nullptr), static_cast<float*>(nullptr), h->playlist->d_rows,
                           static_cast<uint32_t*>(nullptr), 0u, static_cast<const int32_t*>(nullptr), 0, static_cast<int*>(nullptr));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(out_host + done * kDim, h->playlist->d_rows, sizeof(float) * kDim * static_cast<size_t>(c),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MI355REC_OK;
}

}  // extern "C"
