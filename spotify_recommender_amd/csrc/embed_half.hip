// embed_half.hip — libmi355rec_embed_half.so: HALF-PRECISION EMBEDDING TABLES over one device handle of libmi355rec.so
// (include/mi355rec_embed_half.h).  A handle is embed_device.hip.h's table on one device handle plus its storage; what this
// file adds to that host path are the two launches of its kernels (embed_half.hip.h), the create checks and the entry
// points.  The library reaches the catalogue only through the product library's C-ABI: mi355rec_stats (rows, row_base,
// device) and mi355rec_enqueue_scores (s(x) of every row into this library's buffer, on this table's stream).
#include <memory>
#include <new>

#include "embed_device.hip.h"
#include "embed_half.hip.h"
#include "embed_half_request.h"

using namespace mi355;

struct mi355rec_embed_half : EmbedDeviceTable {
    int storage = MI355REC_EMBED_HALF_FP16;
    int64_t queries = 0;
};

namespace {

template <int kDimT, int kStorage>
void launch_scan_as(EmbedDeviceTable* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    hipLaunchKernelGGL((embed_half_scan_kernel<kDimT, kStorage>), dim3(e->grid), dim3(kEmbedBlock), 0, e->stream,
                       static_cast<const uint16_t*>(e->d_table), e->n, e->row_base, e->d_user, d_s, e->d_excl, a, e->d_lists, out_v, out_c);
}

template <int kStorage>
void launch_scan_storage(EmbedDeviceTable* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    switch (e->dim) {
        case 16: launch_scan_as<16, kStorage>(e, a, d_s, out_v, out_c); break;
        case 32: launch_scan_as<32, kStorage>(e, a, d_s, out_v, out_c); break;
        case 64: launch_scan_as<64, kStorage>(e, a, d_s, out_v, out_c); break;
        default: launch_scan_as<128, kStorage>(e, a, d_s, out_v, out_c); break;
    }
}

void launch_scan(EmbedDeviceTable* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    if (static_cast<mi355rec_embed_half*>(e)->storage == MI355REC_EMBED_HALF_FP16) launch_scan_storage<MI355REC_EMBED_HALF_FP16>(e, a, d_s, out_v, out_c);
    else launch_scan_storage<MI355REC_EMBED_HALF_BF16>(e, a, d_s, out_v, out_c);
}

void launch_user(EmbedDeviceTable* e, const EmbedMembers& m) {
    hipLaunchKernelGGL(embed_half_user_kernel, dim3(1), dim3(128), 0, e->stream, static_cast<const uint16_t*>(e->d_table), e->dim,
                       static_cast<mi355rec_embed_half*>(e)->storage, m, e->d_user);
}

constexpr EmbedTableKind kHalfTable = {sizeof(uint16_t), 8, launch_scan, launch_user};

}  // namespace

extern "C" {

int mi355rec_embed_half_create(mi355rec_t* h, const uint16_t* table_words, int64_t n, int dim, int storage, mi355rec_embed_half_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table_words)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_half> e(new (std::nothrow) mi355rec_embed_half());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    char msg[256];
    if (mi355embedhalf::invalid_table(table_words, n, dim, storage, st.rows, msg, sizeof msg)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "%s", msg);
    e->storage = storage;
    const int rc = init_device(e.get(), &kHalfTable, h, st, table_words, n, dim);
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
    out->tile_rows = embed_tile_rows(e->dim, 8);
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
    return enqueue_probe(e, sink_dev, stream);
}

}  // extern "C"
