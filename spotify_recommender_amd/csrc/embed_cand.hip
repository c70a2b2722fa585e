// embed_cand.hip — libmi355rec_embed_cand.so: EMBEDDING CANDIDATE LISTS over one device handle of libmi355rec.so
// (include/mi355rec_embed_cand.h).  A handle is embed_device.hip.h's table on one device handle, borrowed or copied, plus
// the claimed list and the claim bitmap, all allocated at create (the bitmap zeroed there: it is all zero at rest).  An
// enqueue call checks its request on the host, then launches on the CALLER's stream — rank: prepare (only with
// exclusions), mi355rec_enqueue_scores (only with w_audio != 0), claim, gather, merge, finish; scores: the audio launch and
// the gather — records the table's event and returns.  It holds no synchronise, no allocation and no copy from host
// memory; the library reaches the catalogue only through mi355rec_stats and mi355rec_enqueue_scores.
#include <memory>
#include <new>

#include "embed_cand.hip.h"
#include "embed_cand_request.h"
#include "embed_device.hip.h"

using namespace mi355;

namespace {

constexpr int kCandRankLaunches = 4;     // claim, gather, merge, finish
constexpr int kCandScoresLaunches = 1;   // gather

}  // namespace

struct mi355rec_embed_cand : EmbedDeviceTable {
    int storage = MI355REC_EMBED_STREAM_FP32;
    int64_t launches = 0;
    int64_t enqueues = 0;
    // the calls of one table share its work buffers: the event stands behind the last enqueue, on last_stream
    hipEvent_t order_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last_stream = false;
    uint32_t* d_rows = nullptr;    // [MI355REC_EMBED_CAND_MAX] the claimed list of a rank call
    uint32_t* d_claim = nullptr;   // [(n + 31) / 32] one bit per row, all zero between calls

    ~mi355rec_embed_cand() {
        if (device < 0) return;
        DeviceGuard guard(device);
        (void)hipDeviceSynchronize();   // (the work is on the callers' streams; ~EmbedDeviceTable frees what it reads)
        for (void* p : {static_cast<void*>(d_rows), static_cast<void*>(d_claim)})
            if (p) (void)hipFree(p);
        if (order_ev) (void)hipEventDestroy(order_ev);
    }
};

namespace {

constexpr EmbedTableKind kCandF32 = {sizeof(float), 4, nullptr, nullptr};      // (the launches are this file's: they take a stream)
constexpr EmbedTableKind kCandHalf = {sizeof(uint16_t), 8, nullptr, nullptr};

int init_cand_table(mi355rec_embed_cand* e, mi355rec_t* h, const void* table, int64_t n, int dim, int storage, bool borrowed) {
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(e, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    if (st.device < 0) return efail(e, MI355REC_ERR_INVALID_ARG, "embedding candidate lists need a handle on a HIP device (the CPU placement is not served)");
    char msg[256];
    if (mi355embedstream::invalid_table(table, n, dim, storage, st.rows, borrowed, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const bool f32 = storage == MI355REC_EMBED_STREAM_FP32;
    if (borrowed && n > 0) {   // the memory must be the handle's device's
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, table) != hipSuccess) {
            (void)hipGetLastError();
            return efail(e, MI355REC_ERR_INVALID_ARG, "table_dev is not device memory (mi355rec_embed_cand_create copies a host table)");
        }
        if (attr.type != hipMemoryTypeDevice || attr.device != st.device)
            return efail(e, MI355REC_ERR_INVALID_ARG, "table_dev is not memory of the handle's device %d", st.device);
    }
    e->storage = storage;
    e->borrowed_table = borrowed;
    int rc = init_device(e, f32 ? &kCandF32 : &kCandHalf, h, st, table, n, dim);
    if (rc) return rc;
    DeviceGuard guard(e->device);
    EMBED_HIP_TRY(e, hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming));
    if (n > 0 && (rc = dev_alloc(e, &e->d_s, static_cast<size_t>(n)))) return rc;   // (an enqueue call allocates nothing)
    if ((rc = dev_alloc(e, &e->d_rows, static_cast<size_t>(MI355REC_EMBED_CAND_MAX)))) return rc;
    const size_t words = static_cast<size_t>(mi355embedcand::claim_words(n));
    if (words > 0) {
        if ((rc = dev_alloc(e, &e->d_claim, words))) return rc;
        EMBED_HIP_TRY(e, hipMemset(e->d_claim, 0, sizeof(uint32_t) * words));
    }
    return MI355REC_OK;
}

int create(mi355rec_t* h, const void* table, int64_t n, int dim, int storage, bool borrowed, mi355rec_embed_cand_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_cand> e(new (std::nothrow) mi355rec_embed_cand());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = init_cand_table(e.get(), h, table, n, dim, storage, borrowed);
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

// The work buffers are the table's: a call on another stream than the last waits, on the device, for the last one's event.
int order_stream(mi355rec_embed_cand* e, hipStream_t s) {
    if (e->has_last_stream && e->last_stream != s) EMBED_HIP_TRY(e, hipStreamWaitEvent(s, e->order_ev, 0));
    return MI355REC_OK;
}

int record_order(mi355rec_embed_cand* e, hipStream_t s) {
    EMBED_HIP_TRY(e, hipEventRecord(e->order_ev, s));
    e->last_stream = s;
    e->has_last_stream = true;
    return MI355REC_OK;
}

int tile_entries(const mi355rec_embed_cand* e) { return embed_tile_rows(e->dim, e->table_kind->vals); }

// What a gather launch is given beside the table: the list in one of its two shapes and the outputs of one of its two forms.
struct GatherIo {
    const int64_t* ids = nullptr;
    const uint32_t* rows = nullptr;
    int64_t m = 0;
    uint64_t* block_lists = nullptr;
    uint32_t* claim = nullptr;
    float* out_v = nullptr;
    float* out_c = nullptr;
    uint8_t* out_flag = nullptr;
};

template <class Rows, int kDimT>
void launch_gather_as(mi355rec_embed_cand* e, int grid, const float* user_dev, const EmbedArgs& a, const GatherIo& io, hipStream_t s) {
    hipLaunchKernelGGL((embed_cand_kernel<Rows, kDimT>), dim3(grid), dim3(kEmbedBlock), 0, s, static_cast<const typename Rows::Word*>(e->d_table), e->n,
                       e->row_base, io.ids, io.rows, io.m, user_dev, static_cast<const float*>(e->d_s), static_cast<const uint32_t*>(e->d_excl), a,
                       io.block_lists, io.claim, io.out_v, io.out_c, io.out_flag);
}

template <class Rows>
void launch_gather_rows(mi355rec_embed_cand* e, int grid, const float* user_dev, const EmbedArgs& a, const GatherIo& io, hipStream_t s) {
    switch (e->dim) {
        case 16: launch_gather_as<Rows, 16>(e, grid, user_dev, a, io, s); break;
        case 32: launch_gather_as<Rows, 32>(e, grid, user_dev, a, io, s); break;
        case 64: launch_gather_as<Rows, 64>(e, grid, user_dev, a, io, s); break;
        default: launch_gather_as<Rows, 128>(e, grid, user_dev, a, io, s); break;
    }
}

void launch_gather(mi355rec_embed_cand* e, int grid, const float* user_dev, const EmbedArgs& a, const GatherIo& io, hipStream_t s) {
    if (e->storage == MI355REC_EMBED_STREAM_FP32) launch_gather_rows<EmbedRowsF32>(e, grid, user_dev, a, io, s);
    else if (e->storage == MI355REC_EMBED_HALF_FP16) launch_gather_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_FP16>>(e, grid, user_dev, a, io, s);
    else launch_gather_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_BF16>>(e, grid, user_dev, a, io, s);
    ++e->launches;
}

// s(x) of every row of the catalogue into d_s (n > 0).
int enqueue_audio(mi355rec_embed_cand* e, const mi355embedcand::Query& r, hipStream_t s) {
    const int rc = mi355rec_enqueue_scores(e->h, r.audio ? -1 : r.audio_row, r.audio, e->d_s, s);
    if (rc != MI355REC_OK) return efail(e, rc, "mi355rec_enqueue_scores: %s", mi355rec_last_error(e->h));
    ++e->scores_launches;
    ++e->launches;
    return MI355REC_OK;
}

EmbedArgs gather_args(const mi355embedcand::Query& r, bool use_audio, int topk) {
    EmbedArgs a;
    a.w_audio = r.w_audio;
    a.w_embed = r.w_embed;
    a.metric = r.metric;
    a.use_audio = use_audio ? 1 : 0;
    a.n_exclude = r.n_exclude;   // (sorted, with duplicates and no-row words: embed_stream.hip.h says why that is the same list)
    a.topk = topk;
    return a;
}

// The top-N over the distinct listed rows on stream s; the request is checked.
int enqueue_rank(mi355rec_embed_cand* e, const mi355embedcand::Query& r, const mi355rec_embed_stream_result_t& res, hipStream_t s) {
    DeviceGuard guard(e->device);
    int rc = order_stream(e, s);
    if (rc) return rc;
    int eff = 0;   // (an empty list or an empty table: finish writes the padding and nothing else is launched)
    if (e->n > 0 && r.n_candidates > 0) {
        eff = static_cast<int64_t>(r.topn) < e->n ? r.topn : static_cast<int>(e->n);
        if (r.n_exclude > 0) {
            hipLaunchKernelGGL(embed_stream_prepare_kernel, dim3(1), dim3(mi355embedstream::prepare_width(r.n_exclude)), 0, s, r.exclude_dev, r.n_exclude,
                               e->row_base, e->n, e->d_excl, static_cast<int64_t*>(nullptr));
            EMBED_HIP_TRY(e, hipGetLastError());
            ++e->launches;
        }
        if (r.use_audio && (rc = enqueue_audio(e, r, s))) return rc;
        const int64_t claim_blocks = (r.n_candidates + kEmbedCandClaimBlock - 1) / kEmbedCandClaimBlock;
        hipLaunchKernelGGL(embed_cand_claim_kernel, dim3(static_cast<int>(std::min<int64_t>(claim_blocks, kEmbedCandClaimGrid))), dim3(kEmbedCandClaimBlock), 0,
                           s, r.candidates_dev, r.n_candidates, e->row_base, e->n, e->d_claim, e->d_rows);
        EMBED_HIP_TRY(e, hipGetLastError());
        ++e->launches;
        const int grid = mi355embedcand::gather_grid(r.n_candidates, tile_entries(e), e->grid);
        GatherIo io;
        io.rows = e->d_rows;
        io.m = r.n_candidates;
        io.block_lists = e->d_lists;
        io.claim = e->d_claim;
        launch_gather(e, grid, r.user_dev, gather_args(r, r.use_audio, eff), io, s);
        EMBED_HIP_TRY(e, hipGetLastError());
        hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kMergeBlock), 0, s, e->d_lists, grid, eff, static_cast<int64_t>(eff), static_cast<int64_t>(0), eff,
                           e->d_keys, static_cast<int64_t*>(nullptr), static_cast<float*>(nullptr), static_cast<int64_t>(0), static_cast<uint32_t*>(nullptr), 0u);
        EMBED_HIP_TRY(e, hipGetLastError());
        ++e->launches;
    }
    hipLaunchKernelGGL(embed_stream_finish_kernel, dim3(1), dim3(kEmbedStreamFinishBlock), 0, s, e->d_keys, eff, r.topn, res.out_idx_dev, res.out_score_dev,
                       res.out_count_dev);
    EMBED_HIP_TRY(e, hipGetLastError());
    ++e->launches;
    return record_order(e, s);
}

// v, c and the flag of every list entry on stream s; the request is checked and its list is not empty.
int enqueue_values(mi355rec_embed_cand* e, const mi355embedcand::Query& r, const mi355rec_embed_cand_scores_t& res, hipStream_t s) {
    DeviceGuard guard(e->device);
    int rc = order_stream(e, s);
    if (rc) return rc;
    const bool use_audio = r.use_audio && e->n > 0;   // (an empty table: every id is outside it, no row's s is read)
    if (use_audio && (rc = enqueue_audio(e, r, s))) return rc;
    GatherIo io;
    io.ids = r.candidates_dev;
    io.m = r.n_candidates;
    io.out_v = res.out_v_dev;
    io.out_c = res.out_c_dev;
    io.out_flag = res.out_flag_dev;
    launch_gather(e, mi355embedcand::gather_grid(r.n_candidates, tile_entries(e), e->grid), r.user_dev, gather_args(r, use_audio, 1), io, s);
    EMBED_HIP_TRY(e, hipGetLastError());
    return record_order(e, s);
}

}  // namespace

extern "C" {

int mi355rec_embed_cand_create_device(mi355rec_t* h, const void* table_dev, int64_t n, int dim, int storage, mi355rec_embed_cand_t** out) {
    return create(h, table_dev, n, dim, storage, true, out);
}

int mi355rec_embed_cand_create(mi355rec_t* h, const void* table_host, int64_t n, int dim, int storage, mi355rec_embed_cand_t** out) {
    return create(h, table_host, n, dim, storage, false, out);
}

void mi355rec_embed_cand_destroy(mi355rec_embed_cand_t* e) { delete e; }

const char* mi355rec_embed_cand_last_error(const mi355rec_embed_cand_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_cand_enqueue_rank(mi355rec_embed_cand_t* e, const mi355rec_embed_cand_query_t* q, const mi355rec_embed_stream_result_t* res, void* stream) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_cand_query_t full;
    mi355rec_embed_stream_result_t fres;
    mi355embedcand::Query r;
    char msg[256];
    if (mi355embedcand::from_cand_rank(q, res, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const int rc = enqueue_rank(e, r, fres, static_cast<hipStream_t>(stream));
    if (rc == MI355REC_OK) ++e->enqueues;
    return rc;
}

int mi355rec_embed_cand_enqueue_scores(mi355rec_embed_cand_t* e, const mi355rec_embed_cand_query_t* q, const mi355rec_embed_cand_scores_t* res, void* stream) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_cand_query_t full;
    mi355rec_embed_cand_scores_t fres;
    mi355embedcand::Query r;
    char msg[256];
    if (mi355embedcand::from_cand_scores(q, res, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const int rc = r.n_candidates > 0 ? enqueue_values(e, r, fres, static_cast<hipStream_t>(stream)) : MI355REC_OK;   // (an empty list: nothing is launched)
    if (rc == MI355REC_OK) ++e->enqueues;
    return rc;
}

int mi355rec_embed_cand_info(const mi355rec_embed_cand_t* e, mi355rec_embed_cand_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_cand_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_cand_info_t))
        return efail(const_cast<mi355rec_embed_cand_t*>(e), MI355REC_ERR_INVALID_ARG, "embed cand info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_cand_info_t)));
    out->dim = e->dim;
    out->rows = e->n;
    out->device_bytes = e->device_bytes;
    out->tile_rows = tile_entries(e);
    out->grid = e->grid;
    out->device = e->device;
    out->storage = e->storage;
    out->table_dev = e->d_table;
    out->launches = e->launches;
    out->enqueues = e->enqueues;
    out->scores_launches = e->scores_launches;
    out->pass_users = 1;
    out->borrowed = e->borrowed_table ? 1 : 0;
    out->max_candidates = MI355REC_EMBED_CAND_MAX;
    out->rank_launches = kCandRankLaunches;
    out->scores_call_launches = kCandScoresLaunches;
    out->reserved = 0;
    return MI355REC_OK;
}

}  // extern "C"
