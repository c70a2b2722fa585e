// engine_diverse.hip.h — DIVERSIFIED TOP-N on the single-device handle (include/mi355rec_diag.h, "DIVERSIFIED TOP-N"): the
// weighted playlist call's top-`pool`, re-ranked by maximal marginal relevance.  The scan launch of the playlist call
// (playlist_launch, engine_playlist.hip.h), the merge into h->d_keys (no ids or scores are unpacked: the pool never leaves
// the device), then mmr_rerank_kernel (diverse.hip.h) on the same stream, which stores the picks into the handle's pinned
// result slots and raises the completion word: the host waits once.  Also here: a pool passed by value (what a row-sharded
// node does after gathering the pool's rows from its shards) and mi355rec_fetch_rows, both launches of the same kernel.
// (Part of mi355rec.hip's translation unit, included after engine_playlist.hip.h.)
#pragma once

#include <cmath>

#include "diverse.hip.h"
#include "engine_playlist.hip.h"

namespace {

// lambda and pool (the other arguments are the playlist call's, checked there with topn = pool).
int check_diverse(mi355rec* h, float lambda, int pool, int topn) {
    if (std::isnan(lambda) || lambda < 0.0f || lambda > 1.0f)
        return fail(h, MI355REC_ERR_INVALID_ARG, "lambda %g out of [0, 1]", static_cast<double>(lambda));
    if (topn <= 0) return fail(h, MI355REC_ERR_INVALID_ARG, "topn must be positive, got %d", topn);
    if (pool < topn || pool > kMaxTopK)
        return fail(h, MI355REC_ERR_INVALID_ARG, "pool %d out of [topn = %d, %d]", pool, topn, kMaxTopK);
    return MI355REC_OK;
}

// The pinned mmr slots and the device rows of the diversified calls (the playlist state holds them).
int ensure_diverse(mi355rec* h) {
    const int rc = ensure_playlist(h);
    if (rc) return rc;
    mi355rec_playlist* P = h->playlist;
    if (!P->h_mmr) {
        HIP_TRY(h, hipHostMalloc(&P->h_mmr, sizeof(float) * kMaxTopK, hipHostMallocMapped));
        HIP_TRY(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&P->hd_mmr), P->h_mmr, 0));
    }
    if (!P->d_rows) HIP_TRY(h, hipMalloc(&P->d_rows, sizeof(float) * kDim * kMaxTopK));
    return MI355REC_OK;
}

void pad_diverse(int from, int topn, int64_t* out_idx, float* out_score, float* out_mmr) {
    for (int i = from; i < topn; ++i) {
        out_idx[i] = -1;
        if (out_score) out_score[i] = 0.0f;
        if (out_mmr) out_mmr[i] = 0.0f;
    }
}

// The re-rank of the `pool` keys in h->d_keys on h->stream, the wait and the results.  rows: the handle's matrix, or
// (staged) the pool's rows in pool order.
int rerank_and_wait(mi355rec* h, const float* rows, bool staged, int pool, float lambda, int topn, int64_t* out_idx, float* out_score,
                    float* out_mmr, int* out_count) {
    mi355rec_playlist* P = h->playlist;
    const float mu = 1.0f - lambda;
    const uint32_t want = ++h->done_seq ? h->done_seq : ++h->done_seq;   // never 0
    const int block = (pool + 63) & ~63;
    hipLaunchKernelGGL(mmr_rerank_kernel, dim3(1), dim3(block), 0, h->stream, static_cast<const uint64_t*>(h->d_keys), rows, h->n,
                       h->row_base, staged ? 1 : 0, pool, topn, lambda, mu, h->hd_idx, h->hd_score, P->hd_mmr,
                       static_cast<float*>(nullptr), h->hd_done, want);
    HIP_TRY(h, hipGetLastError());
    const int rc = wait_done(h, want);
    if (rc) return rc;
    int c = 0;
    while (c < topn && h->h_idx[c] >= 0) ++c;
    std::memcpy(out_idx, h->h_idx, static_cast<size_t>(topn) * sizeof(int64_t));
    if (out_score) std::memcpy(out_score, h->h_score, static_cast<size_t>(topn) * sizeof(float));
    if (out_mmr) std::memcpy(out_mmr, P->h_mmr, static_cast<size_t>(topn) * sizeof(float));
    if (out_count) *out_count = c;
    return MI355REC_OK;
}

int sync_diverse_query(mi355rec* h, const float* members, const int64_t* local_rows, const float* weights, int k,
                       const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, float lambda, int pool, int topn,
                       int64_t* out_idx, float* out_score, float* out_mmr, int* out_count, int max_exclude = kMaxExclude) {
    if (!out_idx) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    int rc = check_diverse(h, lambda, pool, topn);
    if (rc) return rc;
    DeviceGuard guard(h->device);
    int eff = 0, grid = 0;
    rc = playlist_launch(h, members, local_rows, k, exclude_global, n_exclude, pool, out_idx, max_exclude, filter, weights, &eff, &grid);
    if (rc) return rc;
    if (eff <= 0) {
        pad_diverse(0, topn, out_idx, out_score, out_mmr);
        if (out_count) *out_count = 0;
        return MI355REC_OK;
    }
    rc = ensure_diverse(h);
    if (rc) return rc;
    rc = enqueue_merge(h, h->d_block_lists, grid, eff, eff, h->d_keys, nullptr, nullptr, h->stream);
    if (rc) return rc;
    return rerank_and_wait(h, h->d_feats, false, eff, lambda, topn, out_idx, out_score, out_mmr, out_count);
}

}  // namespace

namespace mi355node {
int query_mean_topn_diverse(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global, int n_exclude,
                            const mi355rec_filter_t* filter, float lambda, int pool, int topn, int64_t* out_idx, float* out_score,
                            float* out_mmr, int* out_count) {
    if (!h || !queries) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    return sync_diverse_query(h, queries, nullptr, weights, k, exclude_global, n_exclude, filter, lambda, pool, topn, out_idx, out_score,
                              out_mmr, out_count, kPlExcludeCap);
}

int rerank_pool(mi355rec_t* h, const int64_t* pool_idx, const float* pool_score, const float* pool_rows, int count, float lambda, int topn,
                int64_t* out_idx, float* out_score, float* out_mmr, int* out_count) {
    if (!h || !pool_idx || !pool_score || !pool_rows || !out_idx) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (count < 1 || count > kMaxTopK || topn < 1 || topn > kMaxTopK)
        return fail(h, MI355REC_ERR_INVALID_ARG, "a pool of %d rows, topn %d: 1 to %d are supported", count, topn, kMaxTopK);
    DeviceGuard guard(h->device);
    int rc = ensure_diverse(h);
    if (!rc) rc = ensure_slots(h, static_cast<size_t>(kMaxTopK));
    if (!rc) rc = sync_api_begin(h);
    if (rc) return rc;
    uint64_t keys[kMaxTopK];
    for (int i = 0; i < count; ++i) keys[i] = pack_key(pool_score[i], static_cast<uint32_t>(pool_idx[i]));
    // (pageable sources: each copy has left the host buffer when the call returns)
    HIP_TRY(h, hipMemcpyAsync(h->d_keys, keys, sizeof(uint64_t) * static_cast<size_t>(count), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->playlist->d_rows, pool_rows, sizeof(float) * kDim * static_cast<size_t>(count), hipMemcpyHostToDevice,
                              h->stream));
    return rerank_and_wait(h, h->playlist->d_rows, true, count, lambda, topn, out_idx, out_score, out_mmr, out_count);
}
}  // namespace mi355node

extern "C" {

int mi355rec_query_mean_topn_diverse(mi355rec_t* h, const float* queries, const float* weights, int k, const int64_t* exclude_global,
                                     int n_exclude, const mi355rec_filter_t* filter, float lambda, int pool, int topn, int64_t* out_idx,
                                     float* out_score, float* out_mmr, int* out_count) {
    if (!h || !queries) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    return sync_diverse_query(h, queries, nullptr, weights, k, exclude_global, n_exclude, filter, lambda, pool, topn, out_idx, out_score,
                              out_mmr, out_count);
}

int mi355rec_query_playlist_topn_diverse(mi355rec_t* h, const int64_t* local_rows, const float* weights, int k,
                                         const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter, float lambda,
                                         int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr, int* out_count) {
    if (!h || !local_rows) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    return sync_diverse_query(h, nullptr, local_rows, weights, k, exclude_global, n_exclude, filter, lambda, pool, topn, out_idx, out_score,
                              out_mmr, out_count);
}

int mi355rec_fetch_rows(mi355rec_t* h, const int64_t* local_rows, int64_t count, float* out_host) {
    if (!h || (count > 0 && (!local_rows || !out_host))) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (count < 0) return fail(h, MI355REC_ERR_INVALID_ARG, "count %lld is negative", (long long)count);
    for (int64_t i = 0; i < count; ++i)
        if (local_rows[i] < 0 || local_rows[i] >= h->n)
            return fail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)local_rows[i]);
    if (count == 0) return MI355REC_OK;
    DeviceGuard guard(h->device);
    int rc = ensure_diverse(h);
    if (!rc) rc = ensure_slots(h, static_cast<size_t>(kMaxTopK));
    if (!rc) rc = sync_api_begin(h);
    if (rc) return rc;
    uint64_t keys[kMaxTopK];
    for (int64_t done = 0; done < count; done += kMaxTopK) {   // one gather launch and one copy back per 1024 rows
        const int c = static_cast<int>(count - done < kMaxTopK ? count - done : kMaxTopK);
        for (int i = 0; i < c; ++i) keys[i] = pack_key(0.0f, static_cast<uint32_t>(h->row_base + local_rows[done + i]));
        HIP_TRY(h, hipMemcpyAsync(h->d_keys, keys, sizeof(uint64_t) * static_cast<size_t>(c), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(mmr_rerank_kernel, dim3(1), dim3((c + 63) & ~63), 0, h->stream, static_cast<const uint64_t*>(h->d_keys),
                           static_cast<const float*>(h->d_feats), h->n, h->row_base, 0, c, 0, 0.0f, 0.0f, static_cast<int64_t*>(nullptr),
                           static_cast<float*>(nullptr), static_cast<float*>(nullptr), h->playlist->d_rows,
                           static_cast<uint32_t*>(nullptr), 0u);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(out_host + done * kDim, h->playlist->d_rows, sizeof(float) * kDim * static_cast<size_t>(c),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return MI355REC_OK;
}

}  // extern "C"
