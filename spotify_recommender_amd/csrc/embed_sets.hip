// embed_sets.hip — libmi355rec_embed_sets.so: RESTRICTED EMBEDDING REQUESTS over one device handle of libmi355rec.so
// (include/mi355rec_embed_sets.h).  A handle is embed_device.hip.h's table on one device handle plus its storage, the sets
// of the request in flight and its counters; a row set is a host bitmap (csrc/embed_sets_request.h) and its device copy.
// What this file adds to the shared host path are the launches of its kernels (embed_sets.hip.h), the counter's word in front of the keys,
// the set calls and the entry points.  The no-launch cases are decided from the host bitmaps before anything is enqueued.
// The library reaches the catalogue only through the product library's C-ABI: mi355rec_stats and mi355rec_enqueue_scores.
#include <memory>
#include <new>

#include "embed_device.hip.h"
#include "embed_sets.hip.h"
#include "embed_sets_request.h"

using namespace mi355;

constexpr int kStorageF32 = -1;

struct mi355rec_embed_sets : EmbedDeviceTable {
    int storage = kStorageF32;
    int64_t queries = 0;
    int64_t tiles_total = 0;
    int64_t launches_skipped = 0;
    int64_t tiles_scored = 0;              // the device counter (the word in front of d_keys, cumulative since create) as last read back
    const uint32_t* cur_only = nullptr;    // the device bitmaps of the request in flight
    const uint32_t* cur_seen = nullptr;
};

struct mi355rec_embed_sets_rowset {
    mi355rec_embed_sets* table = nullptr;
    mi355embedsets::Bitmap bits;
    uint32_t* d_words = nullptr;   // bits.w.size() words on the table's device
};

namespace {

int vals_of(const mi355rec_embed_sets* e) { return e->storage == kStorageF32 ? 4 : 8; }

template <class Rows, int kDimT>
void launch_scan_as(mi355rec_embed_sets* e, const EmbedArgs& a, const float* d_s) {
    hipLaunchKernelGGL((embed_sets_scan_kernel<Rows, kDimT>), dim3(e->grid), dim3(kEmbedBlock), 0, e->stream,
                       static_cast<const typename Rows::Word*>(e->d_table), e->n, e->row_base, e->d_user, d_s, e->d_excl, a, e->d_lists,
                       e->cur_only, e->cur_seen, reinterpret_cast<unsigned long long*>(e->d_keys - 1));
}

template <class Rows>
void launch_scan_rows(mi355rec_embed_sets* e, const EmbedArgs& a, const float* d_s) {
    switch (e->dim) {
        case 16: launch_scan_as<Rows, 16>(e, a, d_s); break;
        case 32: launch_scan_as<Rows, 32>(e, a, d_s); break;
        case 64: launch_scan_as<Rows, 64>(e, a, d_s); break;
        default: launch_scan_as<Rows, 128>(e, a, d_s); break;
    }
}

// The selecting form only: this library has no parity hook (out_v and out_c are null).
void launch_scan(EmbedDeviceTable* t, const EmbedArgs& a, const float* d_s, float*, float*) {
    auto* e = static_cast<mi355rec_embed_sets*>(t);
    const int64_t group = e->dim / vals_of(e);
    e->tiles_total += (e->n * group + kEmbedTileVecs - 1) / kEmbedTileVecs;
    if (e->storage == kStorageF32) launch_scan_rows<EmbedRowsF32>(e, a, d_s);
    else if (e->storage == MI355REC_EMBED_HALF_FP16) launch_scan_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_FP16>>(e, a, d_s);
    else launch_scan_rows<EmbedRowsHalf<MI355REC_EMBED_HALF_BF16>>(e, a, d_s);
}

void launch_user(EmbedDeviceTable* t, const EmbedMembers& m) {
    auto* e = static_cast<mi355rec_embed_sets*>(t);
    if (e->storage == kStorageF32)
        hipLaunchKernelGGL(embed_user_kernel, dim3(1), dim3(128), 0, e->stream, static_cast<const float*>(e->d_table), e->dim, m, e->d_user);
    else
        hipLaunchKernelGGL(embed_half_user_kernel, dim3(1), dim3(128), 0, e->stream, static_cast<const uint16_t*>(e->d_table), e->dim, e->storage, m,
                           e->d_user);
}

// One word in front of the keys: the scored-tile counter, copied back with them.
constexpr EmbedTableKind kSetsTableF32 = {sizeof(float), 4, launch_scan, launch_user, 1};
constexpr EmbedTableKind kSetsTableHalf = {sizeof(uint16_t), 8, launch_scan, launch_user, 1};

int create_table(mi355rec_t* h, const void* table, int64_t n, int dim, int storage, mi355rec_embed_sets_t** out) {
    if (out) *out = nullptr;
    if (!h || !out) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (n < 0 || (n > 0 && !table)) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table or negative n");
    std::unique_ptr<mi355rec_embed_sets> e(new (std::nothrow) mi355rec_embed_sets());
    if (!e) return efail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    mi355rec_stats_t st;
    if (mi355rec_stats(h, &st) != MI355REC_OK) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "mi355rec_stats: %s", mi355rec_last_error(h));
    char msg[256];
    const bool bad = storage == kStorageF32 ? mi355embed::invalid_table(static_cast<const float*>(table), n, dim, st.rows, msg, sizeof msg)
                                            : mi355embedhalf::invalid_table(static_cast<const uint16_t*>(table), n, dim, storage, st.rows, msg, sizeof msg);
    if (bad) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "%s", msg);
    e->storage = storage;
    int rc = init_device(e.get(), storage == kStorageF32 ? &kSetsTableF32 : &kSetsTableHalf, h, st, table, n, dim);
    if (!rc) {
        DeviceGuard guard(e->device);
        const hipError_t err = hipMemset(e->d_keys - 1, 0, sizeof(uint64_t));
        if (err != hipSuccess) rc = efail(e.get(), MI355REC_ERR_HIP, "hipMemset: %s", hipGetErrorString(err));
    }
    if (rc) {
        t_create_error = e->err;
        return rc;
    }
    *out = e.release();
    return MI355REC_OK;
}

// An empty set over the table, with its zeroed device copy.
int new_rowset(mi355rec_embed_sets* e, std::unique_ptr<mi355rec_embed_sets_rowset>* out) {
    std::unique_ptr<mi355rec_embed_sets_rowset> s(new (std::nothrow) mi355rec_embed_sets_rowset());
    if (!s) return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    try {
        s->bits.reset(e->row_base, e->n);
    } catch (const std::bad_alloc&) {
        return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    s->table = e;
    *out = std::move(s);
    return MI355REC_OK;
}

// The whole bitmap to a fresh device copy, synchronously.
int upload_new(mi355rec_embed_sets* e, mi355rec_embed_sets_rowset* s) {
    DeviceGuard guard(e->device);
    const int rc = dev_alloc(e, &s->d_words, s->bits.w.size());
    if (rc) return rc;
    const hipError_t err = hipMemcpy(s->d_words, s->bits.w.data(), sizeof(uint32_t) * s->bits.w.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        (void)hipFree(s->d_words);
        e->device_bytes -= static_cast<int64_t>(sizeof(uint32_t) * s->bits.w.size());
        s->d_words = nullptr;
        return efail(e, MI355REC_ERR_HIP, "hipMemcpy of a row set: %s", hipGetErrorString(err));
    }
    return MI355REC_OK;
}

}  // namespace

extern "C" {

int mi355rec_embed_sets_create(mi355rec_t* h, const float* table_host, int64_t n, int dim, mi355rec_embed_sets_t** out) {
    return create_table(h, table_host, n, dim, kStorageF32, out);
}

int mi355rec_embed_sets_create_half(mi355rec_t* h, const uint16_t* table_words, int64_t n, int dim, int storage, mi355rec_embed_sets_t** out) {
    if (storage == kStorageF32) {   // (create_table's own code for fp32 is no storage of this call)
        if (out) *out = nullptr;
        return efail(nullptr, MI355REC_ERR_INVALID_ARG, "storage %d: MI355REC_EMBED_HALF_FP16 (0) or MI355REC_EMBED_HALF_BF16 (1)", storage);
    }
    return create_table(h, table_words, n, dim, storage, out);
}

void mi355rec_embed_sets_destroy(mi355rec_embed_sets_t* e) { delete e; }

const char* mi355rec_embed_sets_last_error(const mi355rec_embed_sets_t* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int mi355rec_embed_sets_info(const mi355rec_embed_sets_t* e, mi355rec_embed_sets_info_t* out) {
    if (!e || !out) return efail(const_cast<mi355rec_embed_sets_t*>(e), MI355REC_ERR_INVALID_ARG, "null argument");
    if (out->size != sizeof(mi355rec_embed_sets_info_t))
        return efail(const_cast<mi355rec_embed_sets_t*>(e), MI355REC_ERR_INVALID_ARG, "embed sets info of size %u: this library writes %u bytes",
                     static_cast<unsigned>(out->size), static_cast<unsigned>(sizeof(mi355rec_embed_sets_info_t)));
    out->dim = e->dim;
    out->rows = e->n;
    out->device_bytes = e->device_bytes;
    out->tile_rows = embed_tile_rows(e->dim, vals_of(e));
    out->grid = e->grid;
    out->device = e->device;
    out->shards = 1;
    out->queries = e->queries;
    out->scores_launches = e->scores_launches;
    out->storage = e->storage;
    out->reserved = 0;
    out->tiles_total = e->tiles_total;
    out->tiles_scored = e->tiles_scored;
    out->launches_skipped = e->launches_skipped;
    return MI355REC_OK;
}

int mi355rec_embed_sets_rowset_create(mi355rec_embed_sets_t* e, const int64_t* global_ids, int64_t n_ids, mi355rec_embed_sets_rowset_t** out) {
    if (out) *out = nullptr;
    if (!e || !out) return efail(e, MI355REC_ERR_INVALID_ARG, "null argument");
    std::unique_ptr<mi355rec_embed_sets_rowset> s;
    int rc = new_rowset(e, &s);
    if (rc) return rc;
    char msg[256];
    int64_t lo, hi;
    if (!mi355embedsets::add_ids(s->bits, global_ids, n_ids, nullptr, &lo, &hi, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if ((rc = upload_new(e, s.get()))) return rc;
    *out = s.release();
    return MI355REC_OK;
}

int mi355rec_embed_sets_rowset_create_mask(mi355rec_embed_sets_t* e, const uint8_t* mask_bytes, int64_t n, mi355rec_embed_sets_rowset_t** out) {
    if (out) *out = nullptr;
    if (!e || !out) return efail(e, MI355REC_ERR_INVALID_ARG, "null argument");
    std::unique_ptr<mi355rec_embed_sets_rowset> s;
    int rc = new_rowset(e, &s);
    if (rc) return rc;
    char msg[256];
    if (!mi355embedsets::from_mask(s->bits, mask_bytes, n, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if ((rc = upload_new(e, s.get()))) return rc;
    *out = s.release();
    return MI355REC_OK;
}

int mi355rec_embed_sets_rowset_add(mi355rec_embed_sets_rowset_t* s, const int64_t* global_ids, int64_t n_ids) {
    if (!s) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null row set");
    mi355rec_embed_sets* e = s->table;
    char msg[256];
    mi355embedsets::Undo undo;
    const int64_t count = s->bits.count, blo = s->bits.lo, bhi = s->bits.hi;
    int64_t lo, hi;
    try {
        if (!mi355embedsets::add_ids(s->bits, global_ids, n_ids, &undo, &lo, &hi, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    } catch (const std::bad_alloc&) {
        mi355embedsets::undo_add(s->bits, undo, count, blo, bhi);
        return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    if (hi < lo) return MI355REC_OK;   // nothing new
    DeviceGuard guard(e->device);
    // (a query is synchronous and one call at a time per table: no scan reads the words while they are replaced)
    const hipError_t err = hipMemcpy(s->d_words + lo, s->bits.w.data() + lo, sizeof(uint32_t) * static_cast<size_t>(hi - lo + 1), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        mi355embedsets::undo_add(s->bits, undo, count, blo, bhi);
        (void)hipMemcpy(s->d_words + lo, s->bits.w.data() + lo, sizeof(uint32_t) * static_cast<size_t>(hi - lo + 1), hipMemcpyHostToDevice);
        return efail(e, MI355REC_ERR_HIP, "hipMemcpy of a row set: %s", hipGetErrorString(err));
    }
    return MI355REC_OK;
}

int64_t mi355rec_embed_sets_rowset_count(const mi355rec_embed_sets_rowset_t* s) { return s ? s->bits.count : -1; }

void mi355rec_embed_sets_rowset_destroy(mi355rec_embed_sets_rowset_t* s) {
    if (!s) return;
    if (s->d_words) {
        mi355rec_embed_sets* e = s->table;
        DeviceGuard guard(e->device);
        (void)hipFree(s->d_words);
        e->device_bytes -= static_cast<int64_t>(sizeof(uint32_t) * s->bits.w.size());
    }
    delete s;
}

int mi355rec_embed_sets_query(mi355rec_embed_sets_t* e, const mi355rec_embed_query_t* q, const mi355rec_embed_sets_ext_t* ext,
                              const mi355rec_embed_result_t* res) {
    if (!e) return efail(nullptr, MI355REC_ERR_INVALID_ARG, "null table");
    mi355rec_embed_query_t full;
    mi355rec_embed_result_t fres;
    mi355rec_embed_sets_ext_t fext;
    mi355embed::Request r;
    char msg[256];
    if (mi355embed::from_query(q, res, true, e->n, &full, &fres, &r, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if (mi355embedsets::read_ext(ext, &fext, msg, sizeof msg)) return efail(e, MI355REC_ERR_INVALID_ARG, "%s", msg);
    if ((fext.seen && fext.seen->table != e) || (fext.only && fext.only->table != e))
        return efail(e, MI355REC_ERR_INVALID_ARG, "row set of another table");
    ++e->queries;
    const mi355embedsets::Bitmap* seen = fext.seen ? &fext.seen->bits : nullptr;
    const mi355embedsets::Bitmap* only = fext.only ? &fext.only->bits : nullptr;
    if (e->n == 0 || mi355embedsets::answers_nothing(seen, only)) {   // nothing is enqueued
        ++e->launches_skipped;
        mi355embed::write_result(nullptr, 0, r.topn, fres);
        return MI355REC_OK;
    }
    std::vector<uint64_t> keys;
    int count = 0;
    try {
        keys.assign(static_cast<size_t>(r.topn) + 1, 0ull);   // (the counter's word, then the keys)
    } catch (const std::bad_alloc&) {
        return efail(e, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    e->cur_seen = fext.seen ? fext.seen->d_words : nullptr;
    e->cur_only = fext.only ? fext.only->d_words : nullptr;
    const int rc = device_keys(e, r, keys.data() + 1, &count);
    e->cur_seen = e->cur_only = nullptr;
    if (rc) return rc;
    e->tiles_scored = static_cast<int64_t>(keys[0]);
    mi355embed::write_result(keys.data() + 1, count, r.topn, fres);
    return MI355REC_OK;
}

}  // extern "C"
