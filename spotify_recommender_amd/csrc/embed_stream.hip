// embed_stream.hip — libmi355rec_embed_stream.so: STREAMED EMBEDDING REQUESTS over one device handle of libmi355rec.so
// (include/mi355rec_embed_stream.h).  A handle is embed_device.hip.h's table on one device handle, borrowed or copied, plus
// the work buffers of both paths, all allocated at create.  An enqueue call checks its request on the host, then launches on
// the CALLER's stream — prepare (only with exclusions), mi355rec_enqueue_scores (only with w_audio != 0), the scan, the
// merge, finish — records the table's event and returns.  It holds no synchronise, no allocation and no copy from host
// memory; the library reaches the catalogue only through mi355rec_stats and mi355rec_enqueue_scores.
#include <memory>
#include <new>

#include "embed_device.hip.h"
#include "embed_stream.hip.h"
#include "embed_stream_request.h"

using namespace mi355;

namespace {

constexpr int kStreamPassUsers = 8;   // the users of one pass of enqueue_users: embed_batch_scan_kernel<d, 8>

}  // namespace

struct mi355rec_embed_stream : EmbedDeviceTable {
    int storage = MI355REC_EMBED_STREAM_FP32;
    int64_t launches = 0;
    int64_t enqueues = 0;
    // the calls of one table share its work buffers: the event stands behind the last enqueue, on last_stream
    hipEvent_t order_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last_stream = false;
    // enqueue_users (fp32 tables only)
    int batch_grid = 0;
    float* d_users = nullptr;        // [MAX_USERS rounded up to whole passes][dim]
    uint64_t* d_blists = nullptr;    // [pass users][batch_grid][MAX_USERS_TOPN]
    uint64_t* d_bkeys = nullptr;     // [MAX_USERS][MAX_USERS_TOPN]
    uint32_t* d_bexcl = nullptr;     // [MAX_USERS][MAX_EXCLUDE]
    int64_t* d_boff = nullptr;       // [MAX_USERS + 1]

    ~mi355rec_embed_stream() {
        if (device < 0) return;
        DeviceGuard guard(device);
        (void)hipDeviceSynchronize();   // (the work is on the callers' streams; ~EmbedDeviceTable frees what it reads)
        for (void* p : {static_cast<void*>(d_users), static_cast<void*>(d_blists), static_cast<void*>(d_bkeys), static_cast<void*>(d_bexcl),
                        static_cast<void*>(d_boff)})
            if (p) (void)hipFree(p);
        if (order_ev) (void)hipEventDestroy(order_ev);
    }
};

namespace {

constexpr EmbedTableKind kStreamF32 = {sizeof(float), 4, nullptr, nullptr};      // (the launches are this file's: they take a stream)
constexpr EmbedTableKind kStreamHalf = {sizeof(uint16_t), 8, nullptr, nullptr};

int init_stream_table(mi355rec_embed_stream* e, mi355rec_t* h, const void* table, int64_t n, int dim, int storage, bool borrowed) {
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(e, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    if (st.device < 0) return efail(e, MI355REC_ERR_INVALID_ARG, "streamed embedding requests need a handle on a HIP device (the CPU placement is not served)");
    char msg[256];
    if (mi355embedstream::invalid_table(table, n, dim, storage, st.rows, borrowed, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const bool f32 = storage == MI355REC_EMBED_STREAM_FP32;
    if (borrowed && n > 0) {   // the memory must be the handle's device's
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, table) != hipSuccess) {
            (void)hipGetLastError();
            return efail(e, MI355REC_ERR_INVALID_ARG, "table_dev is not device memory (mi355rec_embed_stream_create copies a host table)");
        }
        if (attr.type != hipMemoryTypeDevice || attr.device != st.device)
            return efail(e, MI355REC_ERR_INVALID_ARG, "table_dev is not memory of the handle's device %d", st.device);
    }
    e->storage = storage;
    e->borrowed_table = borrowed;
    int rc = init_device(e, f32 ? &kStreamF32 : &kStreamHalf, h, st, table, n, dim);
    if (rc) return rc;
    DeviceGuard guard(e->device);
    EMBED_HIP_TRY(e, hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming));
    if (n > 0 && (rc = dev_alloc(e, &e->d_s, static_cast<size_t>(n)))) return rc;   // (an enqueue call allocates nothing)
    if (!f32) return MI355REC_OK;
    e->batch_grid = embed_grid(n, dim, 4, e->cus);
    const size_t max_users = (MI355REC_EMBED_STREAM_MAX_USERS + kStreamPassUsers - 1) / kStreamPassUsers * static_cast<size_t>(kStreamPassUsers);
    if ((rc = dev_alloc(e, &e->d_users, max_users * dim))) return rc;
    if ((rc = dev_alloc(e, &e->d_blists, static_cast<size_t>(kStreamPassUsers) * e->batch_grid * MI355REC_EMBED_STREAM_MAX_USERS_TOPN))) return rc;
    if ((rc = dev_alloc(e, &e->d_bkeys, static_cast<size_t>(MI355REC_EMBED_STREAM_MAX_USERS) * MI355REC_EMBED_STREAM_MAX_USERS_TOPN))) return rc;
    if ((rc = dev_alloc(e, &e->d_bexcl, static_cast<size_t>(MI355REC_EMBED_STREAM_MAX_USERS) * MI355REC_EMBED_STREAM_MAX_EXCLUDE))) return rc;
    if ((rc = dev_alloc(e, &e->d_boff, MI355REC_EMBED_STREAM_MAX_USERS + 1))) return rc;
    return MI355REC_OK;
}

int create(mi355rec_t* h, const void* table, int64_t n, int dim, int storage, bool borrowed, mi355rec_embed_stream_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_stream> e(new (std::nothrow) mi355rec_embed_stream());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = init_stream_table(e.get(), h, table, n, dim, storage, borrowed);
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

// The work buffers are the table's: a call on another stream than the last waits, on the device, for the last one's event.
int order_stream(mi355rec_embed_stream* e, hipStream_t s) {
    if (e->has_last_stream && e->last_stream != s) EMBED_HIP_TRY(e, hipStreamWaitEvent(s, e->order_ev, 0));
    return MI355REC_OK;
}

int record_order(mi355rec_embed_stream* e, hipStream_t s) {
    EMBED_HIP_TRY(e, hipEventRecord(e->order_ev, s));
    e->last_stream = s;
    e->has_last_stream = true;
    return MI355REC_OK;
}

int prepare_width(int L) { return mi355embedstream::prepare_width(L); }

template <class Rows, int kDimT>
void launch_scan_as(mi355rec_embed_stream* e, const float* user_dev, const EmbedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((embed_stream_scan_kernel<Rows, kDimT>), dim3(e->grid), dim3(kEmbedBlock), 0, s, static_cast<const typename Rows::Word*>(e->d_table),
                       e->n, e->row_base, user_dev, static_cast<const float*>(e->d_s), static_cast<const uint32_t*>(e->d_excl), a, e->d_lists,
                       static_cast<float*>(nullptr), static_cast<float*>(nullptr));
}

template <class Rows>
void launch_scan_rows(mi355rec_embed_stream* e, const float* user_dev, const EmbedArgs& a, hipStream_t s) {
    switch (e->dim) {
        case 16: launch_scan_as<Rows, 16>(e, user_dev, a, s); break;
        case 32: launch_scan_as<Rows, 32>(e, user_dev, a, s); break;
        case 64: launch_scan_as<Rows, 64>(e, user_dev, a, s); break;
        default: launch_scan_as<Rows, 128>(e, user_dev, a, s); break;
    }
}

void launch_scan(mi355rec_embed_stream* e, const float* user_dev, const EmbedArgs& a, hipStream_t s) {
    if (e->storage == MI355REC_EMBED_STREAM_FP32) launch_scan_rows<EmbedRowsF32>(e, user_dev, a, s);
    else if (e->storage == MI355REC_EMBED_HALF_FP16) launch_scan_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_FP16>>(e, user_dev, a, s);
    else launch_scan_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_BF16>>(e, user_dev, a, s);
}

template <int kDimT>
void launch_batch_scan_dim(mi355rec_embed_stream* e, const float* d_users, const int64_t* d_off, const EmbedBatchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((embed_batch_scan_kernel<kDimT, kStreamPassUsers>), dim3(e->batch_grid), dim3(kEmbedBlock), 0, s,
                       static_cast<const float*>(e->d_table), e->n, e->row_base, d_users, static_cast<const uint32_t*>(e->d_bexcl), d_off, a, e->d_blists);
}

void launch_batch_scan(mi355rec_embed_stream* e, const float* d_users, const int64_t* d_off, const EmbedBatchArgs& a, hipStream_t s) {
    switch (e->dim) {
        case 16: launch_batch_scan_dim<16>(e, d_users, d_off, a, s); break;
        case 32: launch_batch_scan_dim<32>(e, d_users, d_off, a, s); break;
        case 64: launch_batch_scan_dim<64>(e, d_users, d_off, a, s); break;
        default: launch_batch_scan_dim<128>(e, d_users, d_off, a, s); break;
    }
}

void launch_finish(mi355rec_embed_stream* e, const uint64_t* keys, int users, int eff, int topn, const mi355rec_embed_stream_result_t& res, hipStream_t s) {
    hipLaunchKernelGGL(embed_stream_finish_kernel, dim3(users), dim3(kEmbedStreamFinishBlock), 0, s, keys, eff, topn, res.out_idx_dev, res.out_score_dev,
                       res.out_count_dev);
    ++e->launches;
}

// One user on stream s; the request is checked.
int enqueue_one(mi355rec_embed_stream* e, const mi355embedstream::Query& r, const mi355rec_embed_stream_result_t& res, hipStream_t s) {
    DeviceGuard guard(e->device);
    int rc = order_stream(e, s);
    if (rc) return rc;
    const int eff = static_cast<int64_t>(r.topn) < e->n ? r.topn : static_cast<int>(e->n);
    if (e->n > 0) {   // (nothing scans an empty table: finish writes the padding)
        if (r.n_exclude > 0) {
            hipLaunchKernelGGL(embed_stream_prepare_kernel, dim3(1), dim3(prepare_width(r.n_exclude)), 0, s, r.exclude_dev, r.n_exclude, e->row_base, e->n,
                               e->d_excl, static_cast<int64_t*>(nullptr));
            EMBED_HIP_TRY(e, hipGetLastError());
            ++e->launches;
        }
        if (r.use_audio) {
            rc = mi355rec_enqueue_scores(e->h, r.audio ? -1 : r.audio_row, r.audio, e->d_s, s);
            if (rc != MI355REC_OK) return efail(e, rc, "mi355rec_enqueue_scores: %s", mi355rec_last_error(e->h));
            ++e->scores_launches;
            ++e->launches;
        }
        EmbedArgs a;
        a.w_audio = r.w_audio;
        a.w_embed = r.w_embed;
        a.metric = r.metric;
        a.use_audio = r.use_audio ? 1 : 0;
        a.n_exclude = r.n_exclude;   // (sorted, with duplicates and kNoRow words: embed_stream.hip.h says why that is the same list)
        a.topk = eff;
        launch_scan(e, r.user_dev, a, s);
        EMBED_HIP_TRY(e, hipGetLastError());
        hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kMergeBlock), 0, s, e->d_lists, e->grid, eff, static_cast<int64_t>(eff), static_cast<int64_t>(0), eff,
                           e->d_keys, static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr), static_cast<int64_t>(0), static_cast<uint32_t*>(nullptr), 0u);
        EMBED_HIP_TRY(e, hipGetLastError());
        e->launches += 2;
    }
    launch_finish(e, e->d_keys, 1, eff, r.topn, res, s);
    EMBED_HIP_TRY(e, hipGetLastError());
    return record_order(e, s);
}

// Many users on stream s; the request is checked.
int enqueue_many(mi355rec_embed_stream* e, const mi355embedstream::Users& r, const mi355rec_embed_stream_result_t& res, hipStream_t s) {
    DeviceGuard guard(e->device);
    int rc = order_stream(e, s);
    if (rc) return rc;
    const int P = kStreamPassUsers;
    const int eff = static_cast<int64_t>(r.topn) < e->n ? r.topn : static_cast<int>(e->n);
    if (e->n > 0) {
        // the users behind one another in the table's buffer, zero vectors behind the last up to a whole pass
        const size_t given = static_cast<size_t>(r.n_users) * e->dim;
        EMBED_HIP_TRY(e, hipMemcpyAsync(e->d_users, r.users_dev, sizeof(float) * given, hipMemcpyDeviceToDevice, s));
        ++e->launches;
        const int short_by = (P - r.n_users % P) % P;
        if (short_by) {
            EMBED_HIP_TRY(e, hipMemsetAsync(e->d_users + given, 0, sizeof(float) * static_cast<size_t>(short_by) * e->dim, s));
            ++e->launches;
        }
        const bool excluding = r.exclude_dev != nullptr;
        if (excluding) {
            hipLaunchKernelGGL(embed_stream_prepare_kernel, dim3(r.n_users), dim3(prepare_width(r.exclude_len)), 0, s, r.exclude_dev, r.exclude_len,
                               e->row_base, e->n, e->d_bexcl, e->d_boff);
            EMBED_HIP_TRY(e, hipGetLastError());
            ++e->launches;
        }
        for (int user0 = 0; user0 < r.n_users; user0 += P) {
            EmbedBatchArgs a;
            a.w_embed = r.w_embed;
            a.metric = r.metric;
            a.topk = eff;
            a.users = std::min(P, r.n_users - user0);
            launch_batch_scan(e, e->d_users + static_cast<size_t>(user0) * e->dim, excluding ? e->d_boff + user0 : nullptr, a, s);
            EMBED_HIP_TRY(e, hipGetLastError());
            // one merge launch for the pass: workgroup b merges the lists of the pass's user b
            hipLaunchKernelGGL(merge_kernel, dim3(a.users), dim3(kMergeBlock), 0, s, e->d_blists, e->batch_grid, eff, static_cast<int64_t>(eff),
                               static_cast<int64_t>(e->batch_grid) * eff, eff, e->d_bkeys + static_cast<size_t>(user0) * eff, static_cast<int64_t*>(nullptr),
                               static_cast<float*>(nullptr), static_cast<int64_t>(eff), static_cast<uint32_t*>(nullptr), 0u);
            EMBED_HIP_TRY(e, hipGetLastError());
            e->launches += 2;
        }
    }
    launch_finish(e, e->d_bkeys, r.n_users, eff, r.topn, res, s);
    EMBED_HIP_TRY(e, hipGetLastError());
    return record_order(e, s);
}

}  // namespace

extern "C" {

int mi355rec_embed_stream_create_device(mi355rec_t* h, const void* table_dev, int64_t n, int dim, int storage, mi355rec_embed_stream_t** out) {
    return create(h, table_dev, n, dim, storage, true, out);
}

int mi355rec_embed_stream_create(mi355rec_t* h, const void* table_host, int64_t n, int dim, int storage, mi355rec_embed_stream_t** out) {
    return create(h, table_host, n, dim, storage, false, out);
}

void mi355rec_embed_stream_destroy(mi355rec_embed_stream_t* e) { delete e; }

const char* mi355rec_embed_stream_last_error(const mi355rec_embed_stream_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_stream_enqueue_query(mi355rec_embed_stream_t* e, const mi355rec_embed_stream_query_t* q, const mi355rec_embed_stream_result_t* res,
                                        void* stream) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_stream_query_t full;
    mi355rec_embed_stream_result_t fres;
    mi355embedstream::Query r;
    char msg[256];
    if (mi355embedstream::from_stream_query(q, res, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const int rc = enqueue_one(e, r, fres, static_cast<hipStream_t>(stream));
    if (rc == MI355REC_OK) ++e->enqueues;
    return rc;
}

int mi355rec_embed_stream_enqueue_users(mi355rec_embed_stream_t* e, const mi355rec_embed_stream_users_t* q, const mi355rec_embed_stream_result_t* res,
                                        void* stream) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_stream_users_t full;
    mi355rec_embed_stream_result_t fres;
    mi355embedstream::Users r;
    char msg[256];
    if (mi355embedstream::from_stream_users(q, res, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if (e->storage != MI355REC_EMBED_STREAM_FP32)
        return efail(e, MI355REC_ERR_INVALID_ARG, "user batches are served over fp32 tables (this table's storage is %d)", e->storage);
    const int rc = enqueue_many(e, r, fres, static_cast<hipStream_t>(stream));
    if (rc == MI355REC_OK) ++e->enqueues;
    return rc;
}

int mi355rec_embed_stream_info(const mi355rec_embed_stream_t* e, mi355rec_embed_stream_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_stream_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_stream_info_t))
        return efail(const_cast<mi355rec_embed_stream_t*>(e), MI355REC_ERR_INVALID_ARG, "embed stream info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_stream_info_t)));
    out->dim = e->dim;
    out->rows = e->n;
    out->device_bytes = e->device_bytes;
    out->tile_rows = embed_tile_rows(e->dim, e->table_kind->vals);
    out->grid = e->grid;
    out->device = e->device;
    out->storage = e->storage;
    out->table_dev = e->d_table;
    out->launches = e->launches;
    out->enqueues = e->enqueues;
    out->scores_launches = e->scores_launches;
    out->pass_users = kStreamPassUsers;
    out->borrowed = e->borrowed_table ? 1 : 0;
    return MI355REC_OK;
}

}  // extern "C"
