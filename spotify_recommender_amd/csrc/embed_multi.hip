// embed_multi.hip — libmi355rec_embed_multi.so: MULTI-INTEREST EMBEDDING REQUESTS over one device handle of libmi355rec.so
// (include/mi355rec_embed_multi.h).  A handle is embed_device.hip.h's table on one device handle, borrowed or copied, plus
// the audio side's buffer, all allocated at create.  An enqueue call checks its request on the host, then launches on the
// CALLER's stream — prepare (only with exclusions), mi355rec_enqueue_scores (only with w_audio != 0), the scan, the merge,
// finish — records the table's event and returns.  It holds no synchronise, no allocation and no copy from host memory; the
// interests are read where the caller left them; the library reaches the catalogue only through mi355rec_stats and
// mi355rec_enqueue_scores.
#include <memory>
#include <new>

#include "embed_device.hip.h"
#include "embed_multi.hip.h"
#include "embed_multi_request.h"

using namespace mi355;

namespace {

constexpr int kMultiQueryLaunches = 3;   // scan, merge, finish

}  // namespace

struct mi355rec_embed_multi : EmbedDeviceTable {
    int storage = MI355REC_EMBED_STREAM_FP32;
    int64_t launches = 0;
    int64_t enqueues = 0;
    // the calls of one table share its work buffers: the event stands behind the last enqueue, on last_stream
    hipEvent_t order_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last_stream = false;

    ~mi355rec_embed_multi() {
        if (device < 0) return;
        DeviceGuard guard(device);
        (void)hipDeviceSynchronize();   // (the work is on the callers' streams; ~EmbedDeviceTable frees what it reads)
        if (order_ev) (void)hipEventDestroy(order_ev);
    }
};

namespace {

constexpr EmbedTableKind kMultiF32 = {sizeof(float), 4, nullptr, nullptr};      // (the launches are this file's: they take a stream)
constexpr EmbedTableKind kMultiHalf = {sizeof(uint16_t), 8, nullptr, nullptr};

int init_multi_table(mi355rec_embed_multi* e, mi355rec_t* h, const void* table, int64_t n, int dim, int storage, bool borrowed) {
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(e, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    char msg[256];
    if (mi355embedmulti::invalid_handle(st.device, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if (mi355embedstream::invalid_table(table, n, dim, storage, st.rows, borrowed, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const bool f32 = storage == MI355REC_EMBED_STREAM_FP32;
    if (borrowed && n > 0) {   // the memory must be the handle's device's
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, table) != hipSuccess) {
            (void)hipGetLastError();
            return efail(e, MI355REC_ERR_INVALID_ARG, "table_dev is not device memory (mi355rec_embed_multi_create copies a host table)");
        }
        if (attr.type != hipMemoryTypeDevice || attr.device != st.device)
            return efail(e, MI355REC_ERR_INVALID_ARG, "table_dev is not memory of the handle's device %d", st.device);
    }
    e->storage = storage;
    e->borrowed_table = borrowed;
    int rc = init_device(e, f32 ? &kMultiF32 : &kMultiHalf, h, st, table, n, dim);
    if (rc) return rc;
    DeviceGuard guard(e->device);
    EMBED_HIP_TRY(e, hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming));
    if (n > 0 && (rc = dev_alloc(e, &e->d_s, static_cast<size_t>(n)))) return rc;   // (an enqueue call allocates nothing)
    return MI355REC_OK;
}

int create(mi355rec_t* h, const void* table, int64_t n, int dim, int storage, bool borrowed, mi355rec_embed_multi_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_multi> e(new (std::nothrow) mi355rec_embed_multi());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = init_multi_table(e.get(), h, table, n, dim, storage, borrowed);
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

// The work buffers are the table's: a call on another stream than the last waits, on the device, for the last one's event.
int order_stream(mi355rec_embed_multi* e, hipStream_t s) {
    if (e->has_last_stream && e->last_stream != s) EMBED_HIP_TRY(e, hipStreamWaitEvent(s, e->order_ev, 0));
    return MI355REC_OK;
}

int record_order(mi355rec_embed_multi* e, hipStream_t s) {
    EMBED_HIP_TRY(e, hipEventRecord(e->order_ev, s));
    e->last_stream = s;
    e->has_last_stream = true;
    return MI355REC_OK;
}

template <class Rows, int kDimT>
void launch_scan_as(mi355rec_embed_multi* e, const float* interests_dev, const EmbedMultiArgs& m, hipStream_t s) {
    hipLaunchKernelGGL((embed_multi_scan_kernel<Rows, kDimT>), dim3(e->grid), dim3(kEmbedBlock), 0, s, static_cast<const typename Rows::Word*>(e->d_table),
                       e->n, e->row_base, interests_dev, static_cast<const float*>(e->d_s), static_cast<const uint32_t*>(e->d_excl), m, e->d_lists);
}

template <class Rows>
void launch_scan_rows(mi355rec_embed_multi* e, const float* interests_dev, const EmbedMultiArgs& m, hipStream_t s) {
    switch (e->dim) {
        case 16: launch_scan_as<Rows, 16>(e, interests_dev, m, s); break;
        case 32: launch_scan_as<Rows, 32>(e, interests_dev, m, s); break;
        case 64: launch_scan_as<Rows, 64>(e, interests_dev, m, s); break;
        default: launch_scan_as<Rows, 128>(e, interests_dev, m, s); break;
    }
}

void launch_scan(mi355rec_embed_multi* e, const float* interests_dev, const EmbedMultiArgs& m, hipStream_t s) {
    if (e->storage == MI355REC_EMBED_STREAM_FP32) launch_scan_rows<EmbedRowsF32>(e, interests_dev, m, s);
    else if (e->storage == MI355REC_EMBED_HALF_FP16) launch_scan_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_FP16>>(e, interests_dev, m, s);
    else launch_scan_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_BF16>>(e, interests_dev, m, s);
}

// One user's interests on stream s; the request is checked.
int enqueue_one(mi355rec_embed_multi* e, const mi355embedmulti::Query& r, const mi355rec_embed_multi_result_t& res, hipStream_t s) {
    DeviceGuard guard(e->device);
    int rc = order_stream(e, s);
    if (rc) return rc;
    const int eff = static_cast<int64_t>(r.topn) < e->n ? r.topn : static_cast<int>(e->n);
    EmbedMultiFinishArgs f;
    f.table = e->d_table;
    f.n = e->n;
    f.row_base = e->row_base;
    f.interests = r.interests_dev;
    f.audio_s = e->d_s;
    f.m.a.w_audio = r.w_audio;
    f.m.a.w_embed = r.w_embed;
    f.m.a.metric = r.metric;
    f.m.a.use_audio = r.use_audio ? 1 : 0;
    f.m.a.n_exclude = r.n_exclude;   // (sorted, with duplicates and no-row words: embed_stream.hip.h says why that is the same list)
    f.m.a.topk = eff;
    f.m.n_interests = r.n_interests;
    f.storage = e->storage;
    f.dim = e->dim;
    if (e->n > 0) {   // (nothing scans an empty table: finish writes the padding)
        if (r.n_exclude > 0) {
            hipLaunchKernelGGL(embed_stream_prepare_kernel, dim3(1), dim3(mi355embedstream::prepare_width(r.n_exclude)), 0, s, r.exclude_dev, r.n_exclude,
                               e->row_base, e->n, e->d_excl, static_cast<int64_t*>(nullptr));
            EMBED_HIP_TRY(e, hipGetLastError());
            ++e->launches;
        }
        if (r.use_audio) {
            rc = mi355rec_enqueue_scores(e->h, r.audio ? -1 : r.audio_row, r.audio, e->d_s, s);
            if (rc != MI355REC_OK) return efail(e, rc, "mi355rec_enqueue_scores: %s", mi355rec_last_error(e->h));
            ++e->scores_launches;
            ++e->launches;
        }
        launch_scan(e, r.interests_dev, f.m, s);
        EMBED_HIP_TRY(e, hipGetLastError());
        hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kMergeBlock), 0, s, e->d_lists, e->grid, eff, static_cast<int64_t>(eff), static_cast<int64_t>(0), eff,
                           e->d_keys, static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr), static_cast<int64_t>(0), static_cast<uint32_t*>(nullptr), 0u);
        EMBED_HIP_TRY(e, hipGetLastError());
        e->launches += 2;
    }
    hipLaunchKernelGGL(embed_multi_finish_kernel, dim3(1), dim3(kEmbedMultiFinishBlock), 0, s, e->d_keys, eff, r.topn, res.out_idx_dev, res.out_score_dev,
                       res.out_count_dev, res.out_interest_dev, f);
    EMBED_HIP_TRY(e, hipGetLastError());
    ++e->launches;
    return record_order(e, s);
}

}  // namespace

extern "C" {

int mi355rec_embed_multi_create_device(mi355rec_t* h, const void* table_dev, int64_t n, int dim, int storage, mi355rec_embed_multi_t** out) {
    return create(h, table_dev, n, dim, storage, true, out);
}

int mi355rec_embed_multi_create(mi355rec_t* h, const void* table_host, int64_t n, int dim, int storage, mi355rec_embed_multi_t** out) {
    return create(h, table_host, n, dim, storage, false, out);
}

void mi355rec_embed_multi_destroy(mi355rec_embed_multi_t* e) { delete e; }

const char* mi355rec_embed_multi_last_error(const mi355rec_embed_multi_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_multi_enqueue_query(mi355rec_embed_multi_t* e, const mi355rec_embed_multi_query_t* q, const mi355rec_embed_multi_result_t* res,
                                       void* stream) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_multi_query_t full;
    mi355rec_embed_multi_result_t fres;
    mi355embedmulti::Query r;
    char msg[256];
    if (mi355embedmulti::from_multi_query(q, res, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const int rc = enqueue_one(e, r, fres, static_cast<hipStream_t>(stream));
    if (rc == MI355REC_OK) ++e->enqueues;
    return rc;
}

int mi355rec_embed_multi_info(const mi355rec_embed_multi_t* e, mi355rec_embed_multi_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_multi_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_multi_info_t))
        return efail(const_cast<mi355rec_embed_multi_t*>(e), MI355REC_ERR_INVALID_ARG, "embed multi info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_multi_info_t)));
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
    out->pass_users = 1;
    out->borrowed = e->borrowed_table ? 1 : 0;
    out->max_interests = MI355REC_EMBED_MULTI_MAX_INTERESTS;
    out->pass_interests = kEmbedMultiPass;
    out->query_launches = kMultiQueryLaunches;
    out->reserved = 0;
    return MI355REC_OK;
}

}  // extern "C"
