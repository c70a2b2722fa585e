// embed_batch.hip — libmi355rec_embed_batch.so: USER BATCHES over an embedding table (include/mi355rec_embed_batch.h).
//
// The second companion library owns its kernel (embed_batch.hip.h), its device copy of the table and its work buffers, and
// reaches the catalogue only through mi355rec_stats (rows, row_base, device).  A call serves its users in groups of
// pass_users: per group one scan launch and one merge launch (merge_kernel, one workgroup per user of the group), all on
// the table's stream, one synchronise at the end of the call.
#include <memory>
#include <new>

#include "embed_batch.hip.h"
#include "embed_batch_request.h"
#include "embed_device.hip.h"

using namespace mi355;

// Users that share one pass, per dim (DESIGN.md §5.4.22 has the measurements behind the choice).  A build with
// -DMI355REC_EMBED_BATCH_PASS_USERS=P (tools/run_embed_batch.py builds such variants to measure them) uses P at every dim.
#ifdef MI355REC_EMBED_BATCH_PASS_USERS
template <int kDimT>
constexpr int kPassUsers = MI355REC_EMBED_BATCH_PASS_USERS;
#else
template <int kDimT>
constexpr int kPassUsers = 8;
#endif

namespace {

int pass_users_of(int dim) {
    switch (dim) {
        case 16: return kPassUsers<16>;
        case 32: return kPassUsers<32>;
        case 64: return kPassUsers<64>;
        default: return kPassUsers<128>;
    }
}

}  // namespace

struct mi355rec_embed_batch : EmbedHandle {
    int64_t n = 0;
    int dim = 0;
    int pass_users = 0;
    int64_t passes = 0;
    int64_t users_served = 0;
    int device = -1;
    int cus = 0;
    int grid = 0;
    int64_t row_base = 0;
    hipStream_t stream = nullptr;
    float* d_table = nullptr;
    float* d_users = nullptr;      // [MAX_USERS rounded up to whole passes][dim]
    uint64_t* d_lists = nullptr;   // [pass_users][grid][MI355REC_EMBED_BATCH_MAX_TOPN]
    uint64_t* d_keys = nullptr;    // [MAX_USERS][MI355REC_EMBED_BATCH_MAX_TOPN]
    int64_t* d_excl_off = nullptr; // [MAX_USERS + 1]
    uint32_t* d_excl = nullptr;    // the call's exclusion lists (grown on demand)
    size_t excl_cap = 0;

    ~mi355rec_embed_batch() {
        if (device < 0) return;
        DeviceGuard guard(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {static_cast<void*>(d_table), static_cast<void*>(d_users), static_cast<void*>(d_lists), static_cast<void*>(d_keys),
                        static_cast<void*>(d_excl_off), static_cast<void*>(d_excl)})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int init_device(mi355rec_embed_batch* e, mi355rec_t* h, const float* table, int64_t n, int dim) {
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(e, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    char msg[256];
    if (mi355embed::invalid_table(table, n, dim, st.rows, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if (st.device < 0) return efail(e, MI355REC_ERR_INVALID_ARG, "user batches need a handle on a HIP device");
    e->n = n;
    e->dim = dim;
    e->pass_users = pass_users_of(dim);
    e->device = st.device;
    e->cus = st.compute_units > 0 ? st.compute_units : 256;
    e->row_base = st.row_base;
    DeviceGuard guard(e->device);
    e->grid = embed_grid(n, dim, 4, e->cus);
    EMBED_HIP_TRY(e, hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    const size_t max_users = (MI355REC_EMBED_BATCH_MAX_USERS + e->pass_users - 1) / e->pass_users * static_cast<size_t>(e->pass_users);
    int rc = MI355REC_OK;
    if (n > 0 && (rc = dev_alloc(e, &e->d_table, static_cast<size_t>(n) * dim))) return rc;
    if ((rc = dev_alloc(e, &e->d_users, max_users * dim))) return rc;
    if ((rc = dev_alloc(e, &e->d_lists, static_cast<size_t>(e->pass_users) * e->grid * MI355REC_EMBED_BATCH_MAX_TOPN))) return rc;
    if ((rc = dev_alloc(e, &e->d_keys, static_cast<size_t>(MI355REC_EMBED_BATCH_MAX_USERS) * MI355REC_EMBED_BATCH_MAX_TOPN))) return rc;
    if ((rc = dev_alloc(e, &e->d_excl_off, MI355REC_EMBED_BATCH_MAX_USERS + 1))) return rc;
    if (n > 0) EMBED_HIP_TRY(e, hipMemcpy(e->d_table, table, sizeof(float) * static_cast<size_t>(n) * dim, hipMemcpyHostToDevice));
    return MI355REC_OK;
}

template <int kDimT>
void launch_scan_dim(mi355rec_embed_batch* e, const float* d_users, const int64_t* d_off, const EmbedBatchArgs& a) {
    hipLaunchKernelGGL((embed_batch_scan_kernel<kDimT, kPassUsers<kDimT>>), dim3(e->grid), dim3(kEmbedBlock), 0, e->stream, e->d_table, e->n,
                       e->row_base, d_users, e->d_excl, d_off, a, e->d_lists);
}

void launch_scan(mi355rec_embed_batch* e, const float* d_users, const int64_t* d_off, const EmbedBatchArgs& a) {
    switch (e->dim) {
        case 16: launch_scan_dim<16>(e, d_users, d_off, a); break;
        case 32: launch_scan_dim<32>(e, d_users, d_off, a); break;
        case 64: launch_scan_dim<64>(e, d_users, d_off, a); break;
        default: launch_scan_dim<128>(e, d_users, d_off, a); break;
    }
}

// Every user's best keys (sorted descending, 0-padded) into keys[n_users][eff].
int device_keys(mi355rec_embed_batch* e, const mi355embed::BatchRequest& r, int eff, std::vector<uint64_t>* keys) {
    DeviceGuard guard(e->device);
    const int P = e->pass_users;
    const int n_pass = (r.n_users + P - 1) / P;
    std::vector<uint32_t> excl;
    std::vector<int64_t> off;
    mi355embed::normalise_exclusions(r, e->row_base, e->n, &excl, &off);
    const bool excluding = !excl.empty();
    if (excluding) {
        if (excl.size() > e->excl_cap) {
            if (e->d_excl) {
                EMBED_HIP_TRY(e, hipFree(e->d_excl));
                e->device_bytes -= static_cast<int64_t>(sizeof(uint32_t) * e->excl_cap);
                e->d_excl = nullptr;
                e->excl_cap = 0;
            }
            const int rc = dev_alloc(e, &e->d_excl, excl.size());
            if (rc) return rc;
            e->excl_cap = excl.size();
        }
        EMBED_HIP_TRY(e, hipMemcpyAsync(e->d_excl, excl.data(), sizeof(uint32_t) * excl.size(), hipMemcpyHostToDevice, e->stream));
        EMBED_HIP_TRY(e, hipMemcpyAsync(e->d_excl_off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, e->stream));
    }
    // the users, padded with zero vectors to whole passes
    std::vector<float> users(static_cast<size_t>(n_pass) * P * e->dim, 0.0f);
    std::copy(r.users, r.users + static_cast<size_t>(r.n_users) * e->dim, users.begin());
    EMBED_HIP_TRY(e, hipMemcpyAsync(e->d_users, users.data(), sizeof(float) * users.size(), hipMemcpyHostToDevice, e->stream));
    for (int pass = 0; pass < n_pass; ++pass) {
        const int user0 = pass * P;
        EmbedBatchArgs a;
        a.w_embed = r.w_embed;
        a.metric = r.metric;
        a.topk = eff;
        a.users = std::min(P, r.n_users - user0);
        launch_scan(e, e->d_users + static_cast<size_t>(user0) * e->dim, excluding ? e->d_excl_off + user0 : nullptr, a);
        EMBED_HIP_TRY(e, hipGetLastError());
        ++e->passes;
        // one merge launch for the pass: workgroup b merges the gridDim lists of the pass's user b
        hipLaunchKernelGGL(merge_kernel, dim3(a.users), dim3(kMergeBlock), 0, e->stream, e->d_lists, e->grid, eff, static_cast<int64_t>(eff),
                           static_cast<int64_t>(e->grid) * eff, eff, e->d_keys + static_cast<size_t>(user0) * eff, static_cast<int64_t*>(nullptr),
                           static_cast<float*>(nullptr), static_cast<int64_t>(eff), static_cast<uint32_t*>(nullptr), 0u);
        EMBED_HIP_TRY(e, hipGetLastError());
    }
    keys->assign(static_cast<size_t>(r.n_users) * eff, 0ull);
    EMBED_HIP_TRY(e, hipMemcpyAsync(keys->data(), e->d_keys, sizeof(uint64_t) * keys->size(), hipMemcpyDeviceToHost, e->stream));
    EMBED_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return MI355REC_OK;
}

}  // namespace

extern "C" {

int mi355rec_embed_batch_create(mi355rec_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_batch_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table_host)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_batch> e(new (std::nothrow) mi355rec_embed_batch());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = init_device(e.get(), h, table_host, n, dim);
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

void mi355rec_embed_batch_destroy(mi355rec_embed_batch_t* e) { delete e; }

const char* mi355rec_embed_batch_last_error(const mi355rec_embed_batch_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_batch_query(mi355rec_embed_batch_t* e, const mi355rec_embed_batch_query_t* q, const mi355rec_embed_batch_result_t* res) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_batch_query_t full;
    mi355rec_embed_batch_result_t fres;
    mi355embed::BatchRequest r;
    char msg[256];
    if (mi355embed::from_batch_query(q, res, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    const int eff = static_cast<int64_t>(r.topn) < e->n ? r.topn : static_cast<int>(e->n);
    std::vector<uint64_t> keys;
    try {
        if (e->n > 0) {   // (nothing is launched for an empty table)
            const int rc = device_keys(e, r, eff, &keys);
            if (rc) return rc;
        }
    } catch (const std::bad_alloc&) {
        return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    for (int b = 0; b < r.n_users; ++b) {
        const uint64_t* mine = keys.empty() ? nullptr : keys.data() + static_cast<size_t>(b) * eff;
        int count = 0;
        while (mine && count < eff && mine[count] != 0ull) ++count;
        mi355embed::write_batch_result(mine, count, r.topn, b, fres);
    }
    e->users_served += r.n_users;
    return MI355REC_OK;
}

int mi355rec_embed_batch_info(const mi355rec_embed_batch_t* e, mi355rec_embed_batch_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_batch_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_batch_info_t))
        return efail(const_cast<mi355rec_embed_batch_t*>(e), MI355REC_ERR_INVALID_ARG, "embed batch info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_batch_info_t)));
    out->dim = e->dim;
    out->rows = e->n;
    out->device_bytes = e->device_bytes;
    out->tile_rows = embed_tile_rows(e->dim, 4);
    out->grid = e->grid;
    out->device = e->device;
    out->pass_users = e->pass_users;
    out->passes = e->passes;
    out->users_served = e->users_served;
    return MI355REC_OK;
}

}  // extern "C"
