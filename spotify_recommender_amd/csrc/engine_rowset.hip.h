// engine_rowset.hip.h — ROW SETS (include/mi355rec_diag.h, "ROW SETS") on the device side of the host: the set's device copies
// (rowset.h: Part), made and refreshed here for the single handle and, through mi355node::rowset_attach, for every shard of a node
// handle.  No kernel: the bitmap is built on the host (rowset.h) and copied; playlist_launch (engine_playlist.hip.h) hands the copy
// that belongs to its handle's rows to playlist_scan_kernel.  create and add copy synchronously; add uploads every copy whole.
// (Part of mi355rec.hip's translation unit.)
#pragma once

#include <new>

#include "engine_state.hip.h"
#include "rowset.h"

namespace {

constexpr int64_t kRowsetIdEnd = static_cast<int64_t>(UINT32_MAX) + 1;   // a single handle takes any uint32 global id (as exclude_global)

// Slices the host bitmap for `p`, counts it and copies it into p.d_bits (allocated here on first use).  0, or a C-ABI error code
// with why[0..cap) filled.
int rowset_upload(const mi355rec_rowset* s, mi355rowset::Part* p, char* why, size_t cap) {
    const int64_t n = p->hi - p->lo;
    const size_t words = mi355rowset::words_for(n) ? mi355rowset::words_for(n) : 1;
    std::vector<uint32_t> part;
    try {
        part.assign(words, 0u);
    } catch (const std::bad_alloc&) {
        std::snprintf(why, cap, "out of host memory for a row set of %lld rows", (long long)n);
        return MI355REC_ERR_OUT_OF_MEMORY;
    }
    if (n > 0) mi355rowset::slice(s->bits.w.data(), p->lo, p->hi, part.data());
    p->count = mi355rowset::popcount(part.data(), n);
    DeviceGuard guard(p->device);
    hipError_t e = hipSuccess;
    if (!p->d_bits) e = hipMalloc(&p->d_bits, sizeof(uint32_t) * words);
    if (e == hipSuccess) e = hipMemcpy(p->d_bits, part.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice);
    if (e == hipSuccess) return MI355REC_OK;
    (void)hipGetLastError();
    std::snprintf(why, cap, "the row set's bitmap (%lld rows) on device %d: %s", (long long)n, p->device, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? MI355REC_ERR_OUT_OF_MEMORY : MI355REC_ERR_HIP;
}

// The copy of `s` that belongs to the rows `h` scans (its own or, for a lane, its parent's), or null: a set of another handle.
const mi355rowset::Part* rowset_part(const mi355rec* h, const mi355rec_rowset* s) {
    for (const mi355rowset::Part& p : s->parts)
        if (p.rows_key == static_cast<const void*>(h->d_feats) && p.device == h->device && p.hi - p.lo == h->n) return &p;
    return nullptr;
}

void rowset_free(mi355rec_rowset* s) {
    if (!s) return;
    for (mi355rowset::Part& p : s->parts)
        if (p.d_bits) {
            DeviceGuard guard(p.device);
            (void)hipFree(p.d_bits);
        }
    delete s;
}

}  // namespace

namespace mi355node {
// A device copy of rows [lo, hi) of the set beside the rows of `e` (handles that share rows share the copy).
int rowset_attach(mi355rec_rowset* s, mi355rec_t* e, int64_t lo, int64_t hi, char* why, size_t cap) {
    for (const mi355rowset::Part& p : s->parts)
        if (p.rows_key == static_cast<const void*>(e->d_feats) && p.device == e->device && p.lo == lo && p.hi == hi) return MI355REC_OK;
    mi355rowset::Part p;
    p.rows_key = e->d_feats;
    p.device = e->device;
    p.lo = lo;
    p.hi = hi;
    const int rc = rowset_upload(s, &p, why, cap);
    if (rc == MI355REC_OK) {
        try {
            s->parts.push_back(p);
            return MI355REC_OK;
        } catch (const std::bad_alloc&) {
            std::snprintf(why, cap, "out of host memory for a row set");
        }
    }
    if (p.d_bits) {
        DeviceGuard guard(p.device);
        (void)hipFree(p.d_bits);
    }
    return rc == MI355REC_OK ? static_cast<int>(MI355REC_ERR_OUT_OF_MEMORY) : rc;
}
}  // namespace mi355node

extern "C" {

int mi355rec_rowset_create(mi355rec_t* h, const int64_t* global_ids, int64_t n_ids, mi355rec_rowset_t** out) {
    if (!h || !out) return fail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    char why[160];
    if (mi355rowset::invalid_ids(global_ids, n_ids, kRowsetIdEnd, why, sizeof why)) return fail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    mi355rec_rowset* s = new (std::nothrow) mi355rec_rowset();
    if (!s) return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for a row set");
    try {
        s->bits.reset(h->row_base, h->n);
    } catch (const std::bad_alloc&) {
        delete s;
        return fail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for a row set of %lld rows", (long long)h->n);
    }
    s->bits.add(global_ids, n_ids);
    const int rc = mi355node::rowset_attach(s, h, 0, h->n, why, sizeof why);
    if (rc != MI355REC_OK) {
        rowset_free(s);
        return fail(h, rc, "%s", why);
    }
    *out = s;
    return MI355REC_OK;
}

int mi355rec_rowset_add(mi355rec_rowset_t* s, const int64_t* global_ids, int64_t n_ids) {
    if (!s) return fail(nullptr, MI355REC_ERR_INVALID_ARG, "null row set");
    char why[160];
    if (mi355rowset::invalid_ids(global_ids, n_ids, s->node ? s->bits.n : kRowsetIdEnd, why, sizeof why))
        return fail(nullptr, MI355REC_ERR_INVALID_ARG, "%s", why);
    const int64_t before = s->bits.count;
    s->bits.add(global_ids, n_ids);
    if (s->bits.count == before) return MI355REC_OK;   // nothing new: every copy is current
    for (mi355rowset::Part& p : s->parts) {   // every copy whole (a failure on any device fails the call)
        const int rc = rowset_upload(s, &p, why, sizeof why);
        if (rc != MI355REC_OK) return fail(nullptr, rc, "%s", why);
    }
    return MI355REC_OK;
}

int64_t mi355rec_rowset_count(const mi355rec_rowset_t* s) { return s ? s->bits.count : 0; }

void mi355rec_rowset_destroy(mi355rec_rowset_t* s) { rowset_free(s); }

}  // extern "C"
