// embed_half.hip — libmi355rec_embed_half.so: HALF-PRECISION EMBEDDING TABLES over one device handle of libmi355rec.so
// (include/mi355rec_embed_half.h).  The host path of embed.hip for a table on one device handle: the library owns its
// kernels (embed_half.hip.h) and its device buffers and reaches the catalogue only through the product library's C-ABI:
// mi355rec_stats (rows, row_base, device) and mi355rec_enqueue_scores (s(x) of every row into this library's buffer, on
// this table's stream).  One stream, one synchronise per call, nothing is launched for an empty table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "embed_half.hip.h"
#include "embed_half_request.h"

using namespace mi355;

namespace {

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

}  // namespace

struct mi355rec_embed_half {
    std::string err;
    int64_t n = 0;
    int dim = 0;
    int storage = MI355REC_EMBED_HALF_FP16;
    int64_t queries = 0;
    int64_t scores_launches = 0;

    mi355rec_t* h = nullptr;
    int device = -1;
    int cus = 0;
    int grid = 0;
    int64_t row_base = 0;
    hipStream_t stream = nullptr;
    uint16_t* d_table = nullptr;
    float* d_user = nullptr;
    float* d_s = nullptr;          // s(x) of every row (allocated by the first call with w_audio != 0)
    float* d_v = nullptr;          // the parity hook's outputs (allocated by the first _scores call)
    float* d_c = nullptr;
    uint32_t* d_excl = nullptr;
    uint64_t* d_lists = nullptr;   // [grid][MI355REC_MAX_TOPN_FAST]
    uint64_t* d_keys = nullptr;    // [MI355REC_MAX_TOPN_FAST]
    int64_t device_bytes = 0;

    ~mi355rec_embed_half() {
        if (device < 0) return;
        DeviceGuard guard(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {static_cast<void*>(d_table), static_cast<void*>(d_user), static_cast<void*>(d_s), static_cast<void*>(d_v),
                        static_cast<void*>(d_c), static_cast<void*>(d_excl), static_cast<void*>(d_lists), static_cast<void*>(d_keys)})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int efail(mi355rec_embed_half* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    else t_create_error = buf;
    return code;
}

#define EMBED_HALF_HIP_TRY(e, expr)                                                                        \
    do {                                                                                                    \
        const hipError_t err_ = (expr);                                                                     \
        if (err_ != hipSuccess)                                                                             \
            return efail((e), err_ == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP, \
                         "%s: %s", #expr, hipGetErrorString(err_));                                         \
    } while (0)

template <class T>
int dev_alloc(mi355rec_embed_half* e, T** p, size_t count) {
    EMBED_HALF_HIP_TRY(e, hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * count));
    e->device_bytes += static_cast<int64_t>(sizeof(T) * count);
    return MI355REC_OK;
}

int tile_rows_of(int dim) { return kEmbedTileVecs / (dim / 8); }

int init_device(mi355rec_embed_half* e, mi355rec_t* h, const uint16_t* words, int64_t n, int dim, int storage) {
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(e, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    char msg[256];
    if (mi355embedhalf::invalid_table(words, n, dim, storage, st.rows, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    e->h = h;
    e->n = n;
    e->dim = dim;
    e->storage = storage;
    e->device = st.device;
    e->cus = st.compute_units > 0 ? st.compute_units : 256;
    e->row_base = st.row_base;
    DeviceGuard guard(e->device);
    const int64_t n_tiles = (n * (dim / 8) + kEmbedTileVecs - 1) / kEmbedTileVecs;
    // two workgroups per CU, tiles dealt round-robin; at most kMergeMaxLists lists reach the merge
    int64_t grid = std::min<int64_t>(n_tiles, 2 * e->cus);
    grid = std::min<int64_t>(grid, kMergeMaxLists);
    e->grid = static_cast<int>(std::max<int64_t>(grid, 1));
    EMBED_HALF_HIP_TRY(e, hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    int rc = MI355REC_OK;
    if (n > 0 && (rc = dev_alloc(e, &e->d_table, static_cast<size_t>(n) * dim))) return rc;
    if ((rc = dev_alloc(e, &e->d_user, MI355REC_EMBED_MAX_DIM))) return rc;
    if ((rc = dev_alloc(e, &e->d_excl, kEmbedMaxExclude))) return rc;
    if ((rc = dev_alloc(e, &e->d_lists, static_cast<size_t>(e->grid) * MI355REC_MAX_TOPN_FAST))) return rc;
    if ((rc = dev_alloc(e, &e->d_keys, MI355REC_MAX_TOPN_FAST))) return rc;
    if (n > 0) EMBED_HALF_HIP_TRY(e, hipMemcpy(e->d_table, words, sizeof(uint16_t) * static_cast<size_t>(n) * dim, hipMemcpyHostToDevice));
    return MI355REC_OK;
}

template <int kDimT, int kStorage>
void launch_scan_as(mi355rec_embed_half* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    hipLaunchKernelGGL((embed_half_scan_kernel<kDimT, kStorage>), dim3(e->grid), dim3(kEmbedBlock), 0, e->stream, e->d_table, e->n, e->row_base,
                       e->d_user, d_s, e->d_excl, a, e->d_lists, out_v, out_c);
}

template <int kStorage>
void launch_scan_storage(mi355rec_embed_half* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    switch (e->dim) {
        case 16: launch_scan_as<16, kStorage>(e, a, d_s, out_v, out_c); break;
        case 32: launch_scan_as<32, kStorage>(e, a, d_s, out_v, out_c); break;
        case 64: launch_scan_as<64, kStorage>(e, a, d_s, out_v, out_c); break;
        default: launch_scan_as<128, kStorage>(e, a, d_s, out_v, out_c); break;
    }
}

void launch_scan(mi355rec_embed_half* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    if (e->storage == MI355REC_EMBED_HALF_FP16) launch_scan_storage<MI355REC_EMBED_HALF_FP16>(e, a, d_s, out_v, out_c);
    else launch_scan_storage<MI355REC_EMBED_HALF_BF16>(e, a, d_s, out_v, out_c);
}

// What both kinds of call enqueue ahead of the scan: the user vector in d_user and, with w_audio != 0, s(x) in d_s.
int enqueue_inputs(mi355rec_embed_half* e, const mi355embed::Request& r) {
    if (r.user) {
        EMBED_HALF_HIP_TRY(e, hipMemcpyAsync(e->d_user, r.user, sizeof(float) * static_cast<size_t>(e->dim), hipMemcpyHostToDevice, e->stream));
    } else {
        EmbedMembers m;
        for (int i = 0; i < kEmbedMaxMembers; ++i) m.rows[i] = i < r.k ? r.rows[i] : 0;
        m.k = r.k;
        hipLaunchKernelGGL(embed_half_user_kernel, dim3(1), dim3(128), 0, e->stream, e->d_table, e->dim, e->storage, m, e->d_user);
        EMBED_HALF_HIP_TRY(e, hipGetLastError());
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

// The request's best keys (sorted descending) into keys_out[0 .. topn), *count of them non-empty.
int device_keys(mi355rec_embed_half* e, const mi355embed::Request& r, uint64_t* keys_out, int* count) {
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
        EMBED_HALF_HIP_TRY(e, hipMemcpyAsync(e->d_excl, excl.data(), sizeof(uint32_t) * excl.size(), hipMemcpyHostToDevice, e->stream));
    int rc = enqueue_inputs(e, r);
    if (rc) return rc;
    launch_scan(e, args_of(r, static_cast<int>(excl.size()), eff), e->d_s, nullptr, nullptr);
    EMBED_HALF_HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kMergeBlock), 0, e->stream, e->d_lists, e->grid, eff, static_cast<int64_t>(eff),
                       static_cast<int64_t>(0), eff, e->d_keys, static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr),
                       static_cast<int64_t>(0), static_cast<uint32_t*>(nullptr), 0u);
    EMBED_HALF_HIP_TRY(e, hipGetLastError());
    EMBED_HALF_HIP_TRY(e, hipMemcpyAsync(keys_out, e->d_keys, sizeof(uint64_t) * static_cast<size_t>(eff), hipMemcpyDeviceToHost, e->stream));
    EMBED_HALF_HIP_TRY(e, hipStreamSynchronize(e->stream));
    int c = 0;
    while (c < eff && keys_out[c] != 0ull) ++c;
    *count = c;
    return MI355REC_OK;
}

// v and c of every row.
int device_scores(mi355rec_embed_half* e, const mi355embed::Request& r, float* out_v, float* out_c) {
    if (e->n == 0) return MI355REC_OK;
    DeviceGuard guard(e->device);
    int rc = MI355REC_OK;
    if (!e->d_v && (rc = dev_alloc(e, &e->d_v, static_cast<size_t>(e->n)))) return rc;
    if (!e->d_c && (rc = dev_alloc(e, &e->d_c, static_cast<size_t>(e->n)))) return rc;
    rc = enqueue_inputs(e, r);
    if (rc) return rc;
    launch_scan(e, args_of(r, 0, 1), e->d_s, e->d_v, e->d_c);
    EMBED_HALF_HIP_TRY(e, hipGetLastError());
    const size_t bytes = sizeof(float) * static_cast<size_t>(e->n);
    EMBED_HALF_HIP_TRY(e, hipMemcpyAsync(out_v, e->d_v, bytes, hipMemcpyDeviceToHost, e->stream));
    if (out_c) EMBED_HALF_HIP_TRY(e, hipMemcpyAsync(out_c, e->d_c, bytes, hipMemcpyDeviceToHost, e->stream));
    EMBED_HALF_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return MI355REC_OK;
}

}  // namespace

extern "C" {

int mi355rec_embed_half_create(mi355rec_t* h, const uint16_t* table_words, int64_t n, int dim, int storage, mi355rec_embed_half_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table_words)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_half> e(new (std::nothrow) mi355rec_embed_half());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = init_device(e.get(), h, table_words, n, dim, storage);
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

void mi355rec_embed_half_destroy(mi355rec_embed_half_t* e) { delete e; }

const char* mi355rec_embed_half_last_error(const mi355rec_embed_half_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_half_query(mi355rec_embed_half_t* e, const mi355rec_embed_query_t* q, const mi355rec_embed_result_t* res) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_query_t full;
    mi355rec_embed_result_t fres;
    mi355embed::Request r;
    char msg[256];
    if (mi355embed::from_query(q, res, true, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    ++e->queries;
    std::vector<uint64_t> keys;
    int count = 0;
    try {
        keys.assign(static_cast<size_t>(r.topn), 0ull);
    } catch (const std::bad_alloc&) {
        return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    const int rc = device_keys(e, r, keys.data(), &count);
    if (rc) return rc;
    mi355embed::write_result(keys.data(), count, r.topn, fres);
    return MI355REC_OK;
}

int mi355rec_embed_half_scores(mi355rec_embed_half_t* e, const mi355rec_embed_query_t* q, float* out_v_host, float* out_c_host) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    if (!out_v_host) return efail(e, MI355REC_ERR_INVALID_ARG, "null argument");
    mi355rec_embed_query_t full;
    mi355embed::Request r;
    char msg[256];
    if (mi355embed::from_query(q, nullptr, false, e->n, &full, nullptr, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    ++e->queries;
    return device_scores(e, r, out_v_host, out_c_host);
}

int mi355rec_embed_half_info(const mi355rec_embed_half_t* e, mi355rec_embed_half_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_half_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_half_info_t))
        return efail(const_cast<mi355rec_embed_half_t*>(e), MI355REC_ERR_INVALID_ARG, "embed half info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_half_info_t)));
    out->dim = e->dim;
    out->rows = e->n;
    out->device_bytes = e->device_bytes;
    out->tile_rows = tile_rows_of(e->dim);
    out->grid = e->grid;
    out->device = e->device;
    out->shards = 1;
    out->queries = e->queries;
    out->scores_launches = e->scores_launches;
    out->storage = e->storage;
    out->reserved = 0;
    return MI355REC_OK;
}

int mi355rec_embed_half_enqueue_probe(mi355rec_embed_half_t* e, uint32_t* sink_dev, void* stream) {
    if (!e || !sink_dev) return efail(e, MI355REC_ERR_INVALID_ARG, "null argument");
    if (e->n == 0) return MI355REC_OK;
    DeviceGuard guard(e->device);
    const int64_t n_vec = e->n * (e->dim / 8);
    const int grid = static_cast<int>(std::min<int64_t>(2 * e->cus, (n_vec + kEmbedBlock - 1) / kEmbedBlock));
    hipLaunchKernelGGL(embed_probe_kernel, dim3(grid), dim3(kEmbedBlock), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(e->d_table), n_vec, sink_dev);
    EMBED_HALF_HIP_TRY(e, hipGetLastError());
    return MI355REC_OK;
}

}  // extern "C"
