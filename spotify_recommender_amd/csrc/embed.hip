// embed.hip — libmi355rec_embed.so: EMBEDDING TABLES over the handles of libmi355rec.so (include/mi355rec_embed.h).
//
// The companion library owns its kernels (embed.hip.h) and its device buffers and reaches the catalogue only through the
// product library's C-ABI: mi355rec_stats (rows, row_base, device), mi355rec_enqueue_scores (s(x) of every row into this
// library's buffer, on this table's stream), mi355rec_fetch_row (an audio row of another shard) and the node handle's
// accessors.  One mi355rec_embed is one of: a table on one device handle (embed_device.hip.h); the host table of a CPU placement
// (embed_cpu.cpp); or the parent of one device table per shard of a row-sharded node handle, whose keys it merges on the
// host (a replicated placement, and a node handle of one shard, are a device table over the first handle).
#include <functional>
#include <memory>
#include <new>

#include "embed_device.hip.h"

using namespace mi355;

namespace {

enum Kind { kDevice, kCpu, kSharded };

}  // namespace

struct mi355rec_embed : EmbedDeviceTable {   // (the device table is used by kDevice alone)
    int kind = kDevice;
    int64_t queries = 0;

    // ---- the CPU placement ----
    std::vector<float> host_table;
    mi355embed::CpuTable cpu;

    // ---- a row-sharded node handle ----
    mi355rec_sharded_t* node = nullptr;
    std::vector<std::unique_ptr<mi355rec_embed>> shards;   // one per shard that has rows, in row order
    std::vector<mi355rec_t*> shard_handles;
};

namespace {

template <int kDimT>
void launch_scan_dim(EmbedDeviceTable* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    hipLaunchKernelGGL((embed_scan_kernel<kDimT>), dim3(e->grid), dim3(kEmbedBlock), 0, e->stream, static_cast<const float*>(e->d_table), e->n,
                       e->row_base, e->d_user, d_s, e->d_excl, a, e->d_lists, out_v, out_c);
}

void launch_scan(EmbedDeviceTable* e, const EmbedArgs& a, const float* d_s, float* out_v, float* out_c) {
    switch (e->dim) {
        case 16: launch_scan_dim<16>(e, a, d_s, out_v, out_c); break;
        case 32: launch_scan_dim<32>(e, a, d_s, out_v, out_c); break;
        case 64: launch_scan_dim<64>(e, a, d_s, out_v, out_c); break;
        default: launch_scan_dim<128>(e, a, d_s, out_v, out_c); break;
    }
}

void launch_user(EmbedDeviceTable* e, const EmbedMembers& m) {
    hipLaunchKernelGGL(embed_user_kernel, dim3(1), dim3(128), 0, e->stream, static_cast<const float*>(e->d_table), e->dim, m, e->d_user);
}

constexpr EmbedTableKind kF32Table = {sizeof(float), 4, launch_scan, launch_user};

// Fills a fresh kDevice table over `h` (its rows are table[0 .. n)).
int init_f32(mi355rec_embed* e, mi355rec_t* h, const float* table, int64_t n, int dim) {
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(e, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    char msg[256];
    if (mi355embed::invalid_table(table, n, dim, st.rows, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    e->kind = kDevice;
    return init_device(e, &kF32Table, h, st, table, n, dim);
}

// ---- the row-sharded parent: what a shard's table is asked is by VALUE (u and the audio query are formed here) ----

struct ByValue {
    float u[MI355REC_EMBED_MAX_DIM];
    float audio[MI355REC_DIM];
    mi355embed::Request r;
};

// The shard that holds global row `row`, and its local index there.
mi355rec_embed* owner_of(mi355rec_embed* e, int64_t row, int64_t* local, size_t* index) {
    for (size_t i = 0; i < e->shards.size(); ++i) {
        mi355rec_embed* s = e->shards[i].get();
        if (row >= s->row_base && row < s->row_base + s->n) {
            *local = row - s->row_base;
            if (index) *index = i;
            return s;
        }
    }
    return nullptr;
}

int sharded_by_value(mi355rec_embed* e, const mi355embed::Request& r, ByValue* bv) {
    bv->r = r;
    if (!r.user) {
        int rc = MI355REC_OK;
        mi355embed::sum_members(r, e->dim,
                                [&](int64_t row, float* out) {
                                    int64_t local = 0;
                                    mi355rec_embed* s = owner_of(e, row, &local, nullptr);
                                    DeviceGuard guard(s->device);
                                    const float* const src = static_cast<const float*>(s->d_table) + local * e->dim;
                                    if (hipMemcpy(out, src, sizeof(float) * static_cast<size_t>(e->dim), hipMemcpyDeviceToHost) != hipSuccess)
                                        rc = MI355REC_ERR_HIP;
                                },
                                bv->u);
        if (rc) return efail(e, rc, "fetching a member row of the table failed");
        bv->r.user = bv->u;
        bv->r.rows = nullptr;
        bv->r.k = 0;
    }
    if (r.use_audio && !r.audio) {
        int64_t local = 0;
        size_t index = 0;
        owner_of(e, r.audio_row, &local, &index);
        const int rc = mi355rec_fetch_row(e->shard_handles[index], local, bv->audio);
        if (rc != MI355REC_OK) return efail(e, rc, "mi355rec_fetch_row: %s", mi355rec_last_error(e->shard_handles[index]));
        bv->r.audio = bv->audio;
        bv->r.audio_row = -1;
    }
    return MI355REC_OK;
}

int create_checks(const void* handle, const float* table, int64_t n, mi355rec_embed_t** out) {
    if (out) *out = nullptr;
    if (!handle || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    return MI355REC_OK;
}

}  // namespace

extern "C" {

int mi355rec_embed_create(mi355rec_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_t** out) {
    int rc = create_checks(h, table_host, n, out);
    if (rc) return rc;
    std::unique_ptr<mi355rec_embed> e(new (std::nothrow) mi355rec_embed());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    rc = init_f32(e.get(), h, table_host, n, dim);
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

int mi355rec_embed_create_node(mi355rec_sharded_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_t** out) {
    int rc = create_checks(h, table_host, n, out);
    if (rc) return rc;
    std::unique_ptr<mi355rec_embed> e(new (std::nothrow) mi355rec_embed());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    char msg[256];
    const int placement = mi355rec_sharded_placement(h);
    if (placement == MI355REC_PLACEMENT_CPU) {
        const float* rows = nullptr;
        int64_t host_n = 0;
        if (mi355rec_sharded_host_rows(h, &rows, &host_n) != MI355REC_OK)
            return efail(nullptr, MI355REC_ERR_INVALID_ARG, "mi355rec_sharded_host_rows: %s", mi355rec_sharded_last_error(h));
        if (mi355embed::invalid_table(table_host, n, dim, host_n, msg, sizeof msg)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "%s", msg);
        e->kind = kCpu;
        e->n = n;
        e->dim = dim;
        try {
            e->host_table.assign(table_host, table_host + static_cast<size_t>(n) * dim);
        } catch (const std::bad_alloc&) {
            return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
        }
        e->cpu.table = e->host_table.data();
        e->cpu.n = n;
        e->cpu.dim = dim;
        e->cpu.audio_rows = rows;
        *out = e.release();
        return MI355REC_OK;
    }
    int n_shards = 0;
    int64_t total = 0;
    int64_t shard_rows[MI355REC_MAX_SHARDS] = {0};
    if (mi355rec_sharded_info(h, &n_shards, nullptr, &total, nullptr, shard_rows) != MI355REC_OK || n_shards < 1)
        return efail(nullptr, MI355REC_ERR_INVALID_ARG, "mi355rec_sharded_info: %s", mi355rec_sharded_last_error(h));
    if (mi355embed::invalid_table(table_host, n, dim, total, msg, sizeof msg)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if (placement == MI355REC_PLACEMENT_REPLICATED || n_shards == 1) {   // one handle holds every row
        mi355rec_t* first = nullptr;
        if (mi355rec_sharded_shard_handle(h, 0, &first) != MI355REC_OK)
            return efail(nullptr, MI355REC_ERR_INVALID_ARG, "mi355rec_sharded_shard_handle: %s", mi355rec_sharded_last_error(h));
        rc = init_f32(e.get(), first, table_host, n, dim);
        if (rc) {
            t_create_error = e->err;
            return rc;
        }
        *out = e.release();
        return MI355REC_OK;
    }
    e->kind = kSharded;
    e->node = h;
    e->n = n;
    e->dim = dim;
    int64_t lo = 0;
    for (int s = 0; s < n_shards; ++s) {
        const int64_t rows = shard_rows[s];
        if (rows > 0) {
            mi355rec_t* sh = nullptr;
            if (mi355rec_sharded_shard_handle(h, s, &sh) != MI355REC_OK)
                return efail(nullptr, MI355REC_ERR_INVALID_ARG, "mi355rec_sharded_shard_handle: %s", mi355rec_sharded_last_error(h));
            std::unique_ptr<mi355rec_embed> child(new (std::nothrow) mi355rec_embed());
            if (!child) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
            rc = init_f32(child.get(), sh, table_host + lo * dim, rows, dim);
            if (rc == MI355REC_OK && child->row_base != lo) rc = efail(child.get(), MI355REC_ERR_INVALID_ARG, "shard %d starts at row %lld, not %lld", s,
                                                                       static_cast<long long>(child->row_base), static_cast<long long>(lo));
            if (rc) {
                t_create_error = child->err;
                return rc;
            }
            e->shards.push_back(std::move(child));
            e->shard_handles.push_back(sh);
        }
        lo += rows;
    }
    *out = e.release();
    return MI355REC_OK;
}

void mi355rec_embed_destroy(mi355rec_embed_t* e) { delete e; }

const char* mi355rec_embed_last_error(const mi355rec_embed_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_query(mi355rec_embed_t* e, const mi355rec_embed_query_t* q, const mi355rec_embed_result_t* res) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_query_t full;
    mi355rec_embed_result_t fres;
    mi355embed::Request r;
    char msg[256];
    if (mi355embed::from_query(q, res, true, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    ++e->queries;
    if (e->kind == kCpu) {
        if (!mi355embed::cpu_query(e->cpu, r, fres)) return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
        return MI355REC_OK;
    }
    std::vector<uint64_t> keys;
    int count = 0;
    try {
        if (e->kind == kDevice) {
            keys.assign(static_cast<size_t>(r.topn), 0ull);
            const int rc = device_keys(e, r, keys.data(), &count);
            if (rc) return rc;
        } else {
            ByValue bv;
            int rc = sharded_by_value(e, r, &bv);
            if (rc) return rc;
            keys.assign(static_cast<size_t>(r.topn) * e->shards.size(), 0ull);
            for (size_t s = 0; s < e->shards.size(); ++s) {   // (one after the other: v1 does not overlap the shards)
                int c = 0;
                mi355rec_embed* child = e->shards[s].get();
                const int64_t before = child->scores_launches;
                rc = device_keys(child, bv.r, keys.data() + s * static_cast<size_t>(r.topn), &c);
                e->scores_launches += child->scores_launches - before;
                if (rc) return efail(e, rc, "shard on device %d: %s", child->device, child->err.c_str());
            }
            std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());   // exact: a key carries v and the global row
            while (count < r.topn && static_cast<size_t>(count) < keys.size() && keys[static_cast<size_t>(count)] != 0ull) ++count;
        }
    } catch (const std::bad_alloc&) {
        return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    mi355embed::write_result(keys.data(), count, r.topn, fres);
    return MI355REC_OK;
}

int mi355rec_embed_scores(mi355rec_embed_t* e, const mi355rec_embed_query_t* q, float* out_v_host, float* out_c_host) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    if (!out_v_host) return efail(e, MI355REC_ERR_INVALID_ARG, "null argument");
    mi355rec_embed_query_t full;
    mi355embed::Request r;
    char msg[256];
    if (mi355embed::from_query(q, nullptr, false, e->n, &full, nullptr, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    ++e->queries;
    if (e->kind == kCpu) {
        mi355embed::cpu_scores(e->cpu, r, out_v_host, out_c_host);
        return MI355REC_OK;
    }
    if (e->kind == kDevice) return device_scores(e, r, out_v_host, out_c_host);
    ByValue bv;
    int rc = sharded_by_value(e, r, &bv);
    if (rc) return rc;
    for (auto& child : e->shards) {
        const int64_t before = child->scores_launches;
        rc = device_scores(child.get(), bv.r, out_v_host + child->row_base, out_c_host ? out_c_host + child->row_base : nullptr);
        e->scores_launches += child->scores_launches - before;
        if (rc) return efail(e, rc, "shard on device %d: %s", child->device, child->err.c_str());
    }
    return MI355REC_OK;
}

int mi355rec_embed_info(const mi355rec_embed_t* e, mi355rec_embed_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_info_t))
        return efail(const_cast<mi355rec_embed_t*>(e), MI355REC_ERR_INVALID_ARG, "embed info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_info_t)));
    const mi355rec_embed* first = e->kind == kSharded && !e->shards.empty() ? e->shards[0].get() : e;
    out->dim = e->dim;
    out->rows = e->n;
    out->device_bytes = e->device_bytes;
    for (const auto& s : e->shards) out->device_bytes += s->device_bytes;
    out->tile_rows = e->kind == kCpu ? 0 : embed_tile_rows(e->dim, 4);
    out->grid = e->kind == kCpu ? 0 : first->grid;
    out->device = e->kind == kCpu ? -1 : first->device;
    out->shards = e->kind == kSharded ? static_cast<int32_t>(e->shards.size()) : 1;
    out->queries = e->queries;
    out->scores_launches = e->scores_launches;
    return MI355REC_OK;
}

int mi355rec_embed_enqueue_probe(mi355rec_embed_t* e, uint32_t* sink_dev, void* stream) {
    if (!e || !sink_dev) return efail(e, MI355REC_ERR_INVALID_ARG, "null argument");
    if (e->kind != kDevice) return efail(e, MI355REC_ERR_INVALID_ARG, "the probe reads a table over one device handle");
    return enqueue_probe(e, sink_dev, stream);
}

}  // extern "C"
