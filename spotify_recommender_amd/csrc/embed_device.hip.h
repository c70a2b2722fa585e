// embed_device.hip.h — the host path the embedding libraries share (embed.hip, embed_half.hip, embed_batch.hip,
// embed_sets.hip; embed_stream.hip takes the table from it and enqueues on the caller's stream itself; host code
// over the HIP runtime, so no header that the CPU-only programs compile includes it): the device guard, the error function,
// EMBED_HIP_TRY, dev_alloc and the grid rule, and EmbedDeviceTable, a table on one device handle, with its one host path.
// What a library adds to a table is an EmbedTableKind: the size of a stored value, the values per 16-byte load and the two
// launches that name its kernels.  Everything here has internal linkage: the libraries are loaded into one process and share
// nothing but the product library, at link time and at load time.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <string>
#include <vector>

#include "embed.hip.h"
#include "embed_request.h"

namespace {

using namespace mi355;

thread_local std::string t_create_error;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) (void)hipSetDevice(device);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// What every handle of these libraries starts with: its last error and the device memory it holds.
struct EmbedHandle {
    std::string err;
    int64_t device_bytes = 0;
};

// The message goes to the handle, or without one to the thread's create error.
int efail(EmbedHandle* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    else t_create_error = buf;
    return code;
}

#define EMBED_HIP_TRY(e, expr)                                                                              \
    do {                                                                                                    \
        const hipError_t err_ = (expr);                                                                     \
        if (err_ != hipSuccess)                                                                             \
            return efail((e), err_ == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, \
                         "%s: %s", #expr, hipGetErrorString(err_));                                         \
    } while (0)

template <class T>
int dev_alloc(EmbedHandle* e, T** p, size_t count) {
    EMBED_HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * count));
    e->device_bytes += static_cast<int64_t>(sizeof(T) * count);
    return MI355REC_OK;
}

// Rows of one 32 KiB tile, with `vals` stored values per 16-byte load.
int embed_tile_rows(int dim, int vals) { return kEmbedTileVecs / (dim / vals); }

// Two workgroups per CU, tiles dealt round-robin; at most kMergeMaxLists lists (per user) reach the merge.
int embed_grid(int64_t n, int dim, int vals, int cus) {
    const int64_t n_tiles = (n * (dim / vals) + kEmbedTileVecs - 1) / kEmbedTileVecs;
    const int64_t grid = std::min<int64_t>(std::min<int64_t>(n_tiles, 2 * cus), kMergeMaxLists);
    return static_cast<int>(std::max<int64_t>(grid, 1));
}

struct EmbedDeviceTable;

struct EmbedTableKind {
    size_t word_bytes;   // of a stored value
    int vals;            // stored values per 16-byte load
    void (*launch_scan)(EmbedDeviceTable* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c);
    void (*launch_user)(EmbedDeviceTable* e, const EmbedMembers& m);   // d_user from member rows
    // uint64 words a library keeps on the device in front of d_keys: one copy brings them back with the keys, to keys_out[-keys_lead ..)
    int keys_lead = 0;
};

// A table on one device handle (its rows are the handle's, from row_base on).
struct EmbedDeviceTable : EmbedHandle {
    const EmbedTableKind* table_kind = nullptr;
    int64_t n = 0;
    int dim = 0;
    int64_t scores_launches = 0;
    mi355rec_t* h = nullptr;
    int device = -1;
    int cus = 0;
    int grid = 0;
    int64_t row_base = 0;
    hipStream_t stream = nullptr;
    void* d_table = nullptr;
    bool borrowed_table = false;   // d_table is the caller's device memory: never copied into, never freed (embed_stream.hip)
    float* d_user = nullptr;
    float* d_s = nullptr;          // s(x) of every row (allocated by the first call with w_audio != 0)
    float* d_v = nullptr;          // the parity hook's outputs (allocated by the first _scores call)
    float* d_c = nullptr;
    uint32_t* d_excl = nullptr;
    uint64_t* d_lists = nullptr;   // [grid][MI355REC_MAX_TOPN_FAST]
    uint64_t* d_keys = nullptr;    // [MI355REC_MAX_TOPN_FAST], behind the kind's keys_lead words

    ~EmbedDeviceTable() {
        if (device < 0) return;
        DeviceGuard guard(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {borrowed_table ? nullptr : d_table, static_cast<void*>(d_user), static_cast<void*>(d_s), static_cast<void*>(d_v), static_cast<void*>(d_c),
                        static_cast<void*>(d_excl), static_cast<void*>(d_lists), static_cast<void*>(d_keys ? d_keys - table_kind->keys_lead : nullptr)})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Fills a fresh table over `h` (st: its mi355rec_stats) with table[0 .. n); the caller has checked the table against st.rows.
// With borrowed_table set, `table` is device memory of the handle's device and becomes d_table as it is.
int init_device(EmbedDeviceTable* e, const EmbedTableKind* kind, mi355rec_t* h, const mi355rec_stats_t& st, const void* table, int64_t n, int dim) {
    e->table_kind = kind;
    e->h = h;
    e->n = n;
    e->dim = dim;
    e->device = st.device;
    e->cus = st.compute_units > 0 ? st.compute_units : 256;
    e->row_base = st.row_base;
    DeviceGuard guard(e->device);
    e->grid = embed_grid(n, dim, kind->vals, e->cus);
    EMBED_HIP_TRY(e, hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    const size_t table_bytes = kind->word_bytes * static_cast<size_t>(n) * dim;
    int rc = MI355REC_OK;
    if (e->borrowed_table) e->d_table = const_cast<void*>(table);
    else if (n > 0 && (rc = dev_alloc(e, reinterpret_cast<char**>(&e->d_table), table_bytes))) return rc;
    if ((rc = dev_alloc(e, &e->d_user, MI355REC_EMBED_MAX_DIM))) return rc;
    if ((rc = dev_alloc(e, &e->d_excl, kEmbedMaxExclude))) return rc;
    if ((rc = dev_alloc(e, &e->d_lists, static_cast<size_t>(e->grid) * MI355REC_MAX_TOPN_FAST))) return rc;
    if ((rc = dev_alloc(e, &e->d_keys, static_cast<size_t>(kind->keys_lead) + MI355REC_MAX_TOPN_FAST))) return rc;
    e->d_keys += kind->keys_lead;
    if (n > 0 && !e->borrowed_table) EMBED_HIP_TRY(e, hipMemcpy(e->d_table, table, table_bytes, hipMemcpyHostToDevice));
    return MI355REC_OK;
}

// What both kinds of call enqueue ahead of the scan: the user vector in d_user and, with w_audio != 0, s(x) in d_s.
int enqueue_inputs(EmbedDeviceTable* e, const mi355embed::Request& r) {
    if (r.user) {
        EMBED_HIP_TRY(e, hipMemcpyAsync(e->d_user, r.user, sizeof(float) * static_cast<size_t>(e->dim), hipMemcpyHostToDevice, e->stream));
    } else {
        EmbedMembers m;
        for (int i = 0; i < kEmbedMaxMembers; ++i) m.rows[i] = i < r.k ? r.rows[i] : 0;
        m.k = r.k;
        e->table_kind->launch_user(e, m);
        EMBED_HIP_TRY(e, hipGetLastError());
    }
    if (r.use_audio) {
        if (!e->d_s) {
            const int rc = dev_alloc(e, &e->d_s, static_cast<size_t>(e->n));
            if (rc) return rc;
        }
        const int rc = mi355rec_enqueue_scores(e->h, r.audio ? -1 : r.audio_row, r.audio, e->d_s, e->stream);
        if (rc != MI355REC_OK) return efail(e, rc, "mi355rec_enqueue_scores: %s", mi355rec_last_error(e->h));
        ++e->scores_launches;
    }
    return MI355REC_OK;
}

EmbedArgs args_of(const mi355embed::Request& r, int n_exclude, int topk) {
    EmbedArgs a;
    a.w_audio = r.w_audio;
    a.w_embed = r.w_embed;
    a.metric = r.metric;
    a.use_audio = r.use_audio ? 1 : 0;
    a.n_exclude = n_exclude;
    a.topk = topk;
    return a;
}

// The request's best keys of this table (sorted descending) into keys_out[0 .. topn), *count of them non-empty; the kind's
// keys_lead words into keys_out[-keys_lead .. 0).
int device_keys(EmbedDeviceTable* e, const mi355embed::Request& r, uint64_t* keys_out, int* count) {
    *count = 0;
    if (e->n == 0) return MI355REC_OK;
    DeviceGuard guard(e->device);
    const int eff = static_cast<int64_t>(r.topn) < e->n ? r.topn : static_cast<int>(e->n);
    // the exclusion list as the kernel wants it: local rows of this table, sorted, distinct
    std::vector<uint32_t> excl;
    for (int i = 0; i < r.n_exclude; ++i) {
        const int64_t local = r.exclude[i] - e->row_base;
        if (local >= 0 && local < e->n) excl.push_back(static_cast<uint32_t>(local));
    }
    std::sort(excl.begin(), excl.end());
    excl.erase(std::unique(excl.begin(), excl.end()), excl.end());
    if (!excl.empty())
        EMBED_HIP_TRY(e, hipMemcpyAsync(e->d_excl, excl.data(), sizeof(uint32_t) * excl.size(), hipMemcpyHostToDevice, e->stream));
    int rc = enqueue_inputs(e, r);
    if (rc) return rc;
    e->table_kind->launch_scan(e, args_of(r, static_cast<int>(excl.size()), eff), e->d_s, nullptr, nullptr);
    EMBED_HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kMergeBlock), 0, e->stream, e->d_lists, e->grid, eff, static_cast<int64_t>(eff),
                       static_cast<int64_t>(0), eff, e->d_keys, static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr),
                       static_cast<int64_t>(0), static_cast<uint32_t*>(nullptr), 0u);
    EMBED_HIP_TRY(e, hipGetLastError());
    const int lead = e->table_kind->keys_lead;
    EMBED_HIP_TRY(e, hipMemcpyAsync(keys_out - lead, e->d_keys - lead, sizeof(uint64_t) * static_cast<size_t>(lead + eff), hipMemcpyDeviceToHost, e->stream));
    EMBED_HIP_TRY(e, hipStreamSynchronize(e->stream));
    int c = 0;
    while (c < eff && keys_out[c] != 0ull) ++c;
    *count = c;
    return MI355REC_OK;
}

// v and c of every row of this table.
int device_scores(EmbedDeviceTable* e, const mi355embed::Request& r, float* out_v, float* out_c) {
    if (e->n == 0) return MI355REC_OK;
    DeviceGuard guard(e->device);
    int rc = MI355REC_OK;
    if (!e->d_v && (rc = dev_alloc(e, &e->d_v, static_cast<size_t>(e->n)))) return rc;
    if (!e->d_c && (rc = dev_alloc(e, &e->d_c, static_cast<size_t>(e->n)))) return rc;
    rc = enqueue_inputs(e, r);
    if (rc) return rc;
    e->table_kind->launch_scan(e, args_of(r, 0, 1), e->d_s, e->d_v, e->d_c);
    EMBED_HIP_TRY(e, hipGetLastError());
    const size_t bytes = sizeof(float) * static_cast<size_t>(e->n);
    EMBED_HIP_TRY(e, hipMemcpyAsync(out_v, e->d_v, bytes, hipMemcpyDeviceToHost, e->stream));
    if (out_c) EMBED_HIP_TRY(e, hipMemcpyAsync(out_c, e->d_c, bytes, hipMemcpyDeviceToHost, e->stream));
    EMBED_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return MI355REC_OK;
}

// The plain read of the table (embed_probe_kernel) on the caller's stream.
int enqueue_probe(EmbedDeviceTable* e, uint32_t* sink_dev, void* stream) {
    if (e->n == 0) return MI355REC_OK;
    DeviceGuard guard(e->device);
    const int64_t n_vec = e->n * (e->dim / e->table_kind->vals);
    const int grid = static_cast<int>(std::min<int64_t>(2 * e->cus, (n_vec + kEmbedBlock - 1) / kEmbedBlock));
    hipLaunchKernelGGL(embed_probe_kernel, dim3(grid), dim3(kEmbedBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float4*>(e->d_table), n_vec, sink_dev);
    EMBED_HIP_TRY(e, hipGetLastError());
    return MI355REC_OK;
}

}  // namespace
