// sharded.hip — the row-sharded engine behind the C-ABI (include/mi355rec.h,
// "row-sharded catalogue" section): ONE host process drives every GPU of the node.
//
// Replaces the reference's single-device residency (cudaSetDevice(0),
// Recommender.cu:124): shard r owns the contiguous rows [lo_r, hi_r) on device
// devices[r] (an ordinary mi355rec handle created with row_base = lo_r, so its
// keys carry GLOBAL row ids).  Per query every shard runs the fused scan + local
// merge on its own stream, the per-shard top-N key lists meet on device
// devices[0], and the same merge kernel that merges per-workgroup lists merges
// the G per-shard lists.  The result does not depend on G.
//
// Exchange (the only inter-GPU step; 800 B per shard at top-100):
//   PEER  every shard's merge kernel STORES its keys straight into the gather
//         buffer on device 0 through a peer mapping (xGMI point-to-point), an
//         event per shard orders device 0's merge behind them.  No collective, no
//         copy launch.  Default when every device can map device 0's memory.
//   RCCL  one ncclAllGather of topn x batch uint64 keys per rank, issued by that rank's
//         WORKER THREAD on its own stream (communicators from ncclCommInitAll: one per
//         device, one thread per communicator — RCCL's one-thread-per-rank pattern, so no
//         ncclGroupStart/End is involved; the exchange BASELINE.json's north_star names).
//         librccl is opened lazily, only for this transport.
// This layer is host orchestration over the single-device C-ABI and the HIP
// runtime: it launches no kernel of its own.
//
// Two ways in:
//   * synchronous calls (mi355rec_sharded_query_*): what Recommender::recommendByIndex
//     maps to.  One shard -> straight to that shard's handle.  More: scan + local merge per
//     shard, exchange, merge on the first device straight into mapped host memory, ONE
//     host wait (the first device's stream; everything it depends on is ordered by events).
//   * the STREAM (mi355rec_sharded_enqueue_* / _flush / _wait): a serving loop.  One streamed
//     scan launch per shard per query, one exchange + one batched merge per WINDOW of
//     queries, tickets instead of host waits.
// Host threads.  With more than one shard every shard has a WORKER thread that owns its device context,
// its stream and its single-device handle: the caller's thread only posts small task records (a
// single-producer ring per worker) and the workers issue the HIP launches in parallel — one launch per
// shard per query costs the caller ~0.1 us instead of G x ~5 us, and a synchronous query on G GPUs pays
// one shard's launch chain, not G of them.  Cross-shard ordering stays on the device (one event per shard,
// or the collective); the only host-side hand-off is "shard r has RECORDED its event" before the first
// device's worker makes its stream wait for it.  With one shard there are no threads at all.
// A query by ROW never comes back to the host: every shard's kernels read its 48 bytes from
// the owning shard's memory through the peer mapping (checked once at create time against
// the by-value path; without all-pairs peer access the row is fetched once per query).
// REQUESTS (the playlist family of include/mi355rec_diag.h) on a row-sharded catalogue are driven by the caller's thread: every shard
// answers with its own leading keys and ONE host merge makes the node's answer of them (merge_over_shards in node_state.hip.h, over
// the accumulator of shard_merge.h): an any-of request's member indices and a bounded request's totals travel through that merge.
// Whatever changes the handle under the stream (window, window mode, topn, rows) goes through ONE pair in node_stream.hip.h:
// quiesce() closes the open window, drains the workers and waits for every shard's stream; reset_stream() drops the stream's
// buffers and empties its ring.  Shard::lane, set at create time, marks a replica that shares a device — and so its rows and side
// data — with an earlier one.
//
// PLACEMENT (mi355rec_create_placed).  Row sharding is what north_star specifies and the only way to a lower
// latency once a scan is longer than its launches; but a shard below ~4 M rows is launch-bound (measured on one
// MI355X, streamed queries over the 8-bit replica: 12.1 us per query at 1.25 M rows, 15.4 at 3 M, 24.4 at 10 M, 207
// at 100 M — 11 us of fixed cost + 1.95 us per million rows), and every query of a sharded catalogue pays the
// exchange on top.  So
//   SHARDED     rows split over G devices; G given, or (AUTO) as many as keep >= 4 M rows per shard: 1 for the 114 k
//               catalogue of BASELINE configs[0] and up to 7.9 M rows, 2 at 10 M, all 8 from 32 M rows on;
//   REPLICATED  every device holds ALL rows (840 MB at 10 M rows with both replicas) and serves whole WINDOWS of the
//               stream by itself, round-robin: no exchange, no merge across devices, queries/s scale with the
//               devices for any catalogue that fits one.  Synchronous calls go to the replicas in turn.
// A "shard" of a replicated handle is a full replica (lo = 0, hi = n).
#include <cmath>

#include "candidates.h"
#include "node_stream.hip.h"

extern "C" {

const char* mi355rec_sharded_last_error(const mi355rec_sharded_t* h) {
    return h ? h->err.c_str() : g_sharded_error.c_str();
}

void mi355rec_sharded_destroy(mi355rec_sharded_t* h) {
    if (!h) return;
    if (h->cpu) {
        mi355cpu::node_destroy(h->cpu);
        delete h;
        return;
    }
    DeviceRestore restore;
    stop_workers(h);   // they finish what has been posted first
    for (Shard& s : h->shards) {
        if (hipSetDevice(s.device) != hipSuccess) continue;
        if (s.stream) (void)hipStreamSynchronize(s.stream);
    }
    free_stream(h);
    for (size_t i = 0; i < h->r_merged.size(); ++i) {
        if (!h->r_merged[i]) continue;
        if (hipSetDevice(h->shards[i % h->shards.size()].device) == hipSuccess) (void)hipEventDestroy(h->r_merged[i]);
    }
    for (Shard& s : h->shards) {
        if (hipSetDevice(s.device) != hipSuccess) continue;
        if (s.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(s.comm);
        if (s.engine) mi355rec_destroy(s.engine);
        if (s.local_keys) (void)hipFree(s.local_keys);
        if (s.gathered) (void)hipFree(s.gathered);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.stream && s.owns_stream) (void)hipStreamDestroy(s.stream);
    }
    if (!h->shards.empty() && hipSetDevice(h->shards[0].device) == hipSuccess) {
        if (h->gather0) (void)hipFree(h->gather0);
        if (h->d_keys) (void)hipFree(h->d_keys);
        if (h->d_idx) (void)hipFree(h->d_idx);
        if (h->d_score) (void)hipFree(h->d_score);
        if (h->h_idx) (void)hipHostFree(h->h_idx);
        if (h->h_score) (void)hipHostFree(h->h_score);
        for (Window& w : h->win)
            if (w.merged) (void)hipEventDestroy(w.merged);
    }
    delete h;
}

}  // extern "C"

namespace {

// Shard r of a SHARDED handle holds its balanced block of rows; of a REPLICATED one, all of them.
int create_on(const float* feats_host, int64_t n, int dim, const int* devices, int n_shards, bool replicated,
              mi355rec_sharded_t** out) {
    if (out) *out = nullptr;
    if (!out || !feats_host || !devices) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
    if (dim != MI355REC_DIM) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "dim must be %d, got %d", MI355REC_DIM, dim);
    if (n < 1 || n > 0xfffffffell) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "rows %lld out of range", (long long)n);
    if (n_shards < 1 || n_shards > MI355REC_MAX_SHARDS)
        return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "n_shards must be in [1, %d], got %d", MI355REC_MAX_SHARDS, n_shards);
    const int visible = mi355rec_device_count();
    if (visible <= 0)
        return sfail(nullptr, MI355REC_ERR_NO_DEVICE, "no HIP device visible: the MI355X engine has no CPU fallback");
    for (int r = 0; r < n_shards; ++r)
        if (devices[r] < 0 || devices[r] >= visible)
            return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "device %d not in [0,%d)", devices[r], visible);

    DeviceRestore restore;
    mi355rec_sharded* h = new mi355rec_sharded();
    h->n = n;
    h->replicated = replicated;
    h->shards.resize(n_shards);
    auto bail = [&](int code) {
        const std::string keep = g_sharded_error;
        mi355rec_sharded_destroy(h);
        g_sharded_error = keep;
        return code;
    };
    const int root = devices[0];
    for (int r = 0; r < n_shards; ++r) {
        Shard& s = h->shards[r];
        s.device = devices[r];
        if (replicated) {
            s.lo = 0;
            s.hi = n;
        } else {
            bounds(n, n_shards, r, s.lo, s.hi);
        }
        if (hipSetDevice(s.device) != hipSuccess) return bail(sfail(nullptr, MI355REC_ERR_HIP, "hipSetDevice(%d) failed", s.device));
        // a replica on a device that already holds one is a LANE of it (mi355rec_create_lane: the same rows and replicas,
        // own stream state): listing a device twice buys the overlap of two chains of launches, not a second copy
        int same = -1;
        for (int p = 0; p < r && replicated && same < 0; ++p)
            if (h->shards[p].device == s.device) same = p;
        s.lane = same >= 0;
        const int rc = same >= 0 ? mi355rec_create_lane(h->shards[same].engine, &s.engine)
                                 : mi355rec_create(s.hi > s.lo ? feats_host + s.lo * MI355REC_DIM : nullptr, s.hi - s.lo, dim, s.device,
                                                   s.lo, &s.engine);
        if (rc != MI355REC_OK) return bail(sfail(nullptr, rc, "shard %d on device %d: %s", r, s.device, mi355rec_last_global_error()));
        (void)mi355rec_set_stream_pairing(s.engine, MI355REC_PAIRING_OFF);   // (a node's windows run one call behind: its shards do not pair)
        // The shard works on the stream its engine was created with: for a lane that is the stream mi355rec_create_lane CHOSE
        // because kernels on it run beside the first replica's (a hardware queue of its own) — a stream made here would be
        // bound to whichever queue is next, possibly the same one.
        s.stream = static_cast<hipStream_t>(mi355rec_own_stream(s.engine));
        s.owns_stream = false;
        if (!s.stream || hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess)
            return bail(sfail(nullptr, MI355REC_ERR_HIP, "stream / event creation on device %d failed", s.device));
    }
    // Peer mappings.  Stores into the first device's gather buffers need ITS memory mapped on every
    // other device (PEER transport); queries by row need every device's rows mapped on every other.
    // (Replicas never read or write each other's memory.)
    for (int a = 0; a < n_shards && !replicated; ++a) {
        for (int b = 0; b < n_shards; ++b) {
            const int da = devices[a], db = devices[b];
            if (da == db) continue;
            bool ok = false;
            int can = 0;
            if (hipSetDevice(da) == hipSuccess && hipDeviceCanAccessPeer(&can, da, db) == hipSuccess && can) {
                const hipError_t e = hipDeviceEnablePeerAccess(db, 0);
                ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            }
            (void)hipGetLastError();
            if (!ok) {
                h->peer_rows = false;
                if (db == root) h->peer_ok = false;
            }
        }
    }
    if (hipSetDevice(root) != hipSuccess) return bail(sfail(nullptr, MI355REC_ERR_HIP, "hipSetDevice(%d) failed", root));
    for (Window& w : h->win)
        if (hipEventCreateWithFlags(&w.merged, hipEventDisableTiming) != hipSuccess)
            return bail(sfail(nullptr, MI355REC_ERR_HIP, "event creation on device %d failed", root));
    h->transport = h->peer_ok ? MI355REC_TRANSPORT_PEER : MI355REC_TRANSPORT_RCCL;
    if (replicated) {   // one "results are in host memory" event per (ring entry, replica), on the replica's device
        h->r_merged.assign(static_cast<size_t>(kStreamDepth) * n_shards, nullptr);
        for (int w = 0; w < kStreamDepth; ++w)
            for (int r = 0; r < n_shards; ++r)
                if (hipSetDevice(devices[r]) != hipSuccess ||
                    hipEventCreateWithFlags(&h->r_merged[static_cast<size_t>(w) * n_shards + r], hipEventDisableTiming) != hipSuccess)
                    return bail(sfail(nullptr, MI355REC_ERR_HIP, "event creation on device %d failed", devices[r]));
    }

    if (n_shards > 1) {   // one worker per shard (none for a single shard: its calls are made by the caller)
        for (int r = 0; r < n_shards; ++r) {
            h->workers.emplace_back(new Worker());
            h->workers.back()->ring.resize(Worker::kCap);
        }
        for (int r = 0; r < n_shards; ++r) h->workers[r]->th = std::thread(worker_main, h, r);
    }

    // Queries by row through the peer mapping have to give the by-value path's keys: one query
    // per shard boundary, checked here, once, on real multi-device placements (a mismatch or an
    // error switches the pointer path off for this handle; mi355rec_sharded_info's note says so).
    bool distinct = false;
    for (int r = 1; r < n_shards; ++r) distinct = distinct || devices[r] != devices[0];
    if (replicated) {
        // nothing to check: a replica reads its own rows
    } else if (distinct && h->peer_rows && n >= 2) {
        const int topn = n - 1 < 16 ? static_cast<int>(n - 1) : 16;
        std::vector<int64_t> i_ptr(topn), i_val(topn);
        std::vector<float> s_ptr(topn), s_val(topn);
        for (int r = 0; r < n_shards && h->peer_rows; ++r) {
            const Shard& s = h->shards[r];
            if (s.hi == s.lo) continue;
            const int64_t row = s.hi - 1;
            int c0 = 0, c1 = 0;
            int rc = mi355rec_sharded_query_row_topn(h, row, topn, i_ptr.data(), s_ptr.data(), &c0);
            h->peer_rows = false;
            const int rc2 = mi355rec_sharded_query_row_topn(h, row, topn, i_val.data(), s_val.data(), &c1);
            h->peer_rows = true;
            if (rc2 != MI355REC_OK) return bail(sfail(nullptr, rc2, "self-check query failed: %s", h->err.c_str()));
            if (rc != MI355REC_OK || c0 != c1 || i_ptr != i_val ||
                std::memcmp(s_ptr.data(), s_val.data(), sizeof(float) * topn) != 0) {
                h->peer_rows = false;
                h->note = "queries by row travel by value: reading a row through the peer mapping did not reproduce the by-value result";
            }
        }
    } else if (!h->peer_rows) {
        h->note = "queries by row travel by value: no all-pairs peer access between the shards' devices";
    }
    *out = h;
    return MI355REC_OK;
}

// ---- PER-ROW SIDE DATA: labels, groups, priors (the setters below) ----
// One attribute on every shard that owns side data, all or nothing.  The caller's thread drives every shard itself (the
// workers are drained first); a replica on a device that already holds one is a lane of it and shares that one's side data,
// so it is skipped.  set_shard(engine, shard) sets the attribute from the shard's slice, set_shard(engine, nullptr) drops it:
// where one shard fails it is dropped on every shard, so that none keeps what the others do not have.
template <class SetShard>
int set_on_every_shard(mi355rec_sharded_t* h, const char* noun, SetShard set_shard) {
    DeviceRestore restore;
    int rc = drain_workers(h);
    if (rc) return rc;
    for (Shard& s : h->shards) {
        if (s.lane) continue;
        S_HIP(h, hipSetDevice(s.device));
        rc = set_shard(s.engine, &s);
        if (rc != MI355REC_OK) {
            const std::string why = mi355rec_last_error(s.engine);
            for (Shard& o : h->shards)
                if (hipSetDevice(o.device) == hipSuccess) (void)set_shard(o.engine, nullptr);
            return sfail(h, rc, "shard on device %d: %s (the %s were dropped on every shard)", s.device, why.c_str(), noun);
        }
    }
    return MI355REC_OK;
}

}  // namespace

extern "C" {

int mi355rec_create_sharded_on(const float* feats_host, int64_t n, int dim, const int* devices, int n_shards,
                               mi355rec_sharded_t** out) {
    return create_on(feats_host, n, dim, devices, n_shards, false, out);
}

// How many devices a row-sharded catalogue of n rows is spread over when the caller does not say (see "PLACEMENT"
// at the top): as many as keep at least kRowsPerShardAuto rows per shard — a smaller shard is launch-bound, and
// every further shard adds to the exchange.
constexpr int64_t kRowsPerShardAuto = 4000000;

int mi355rec_auto_shards(int64_t n, int visible_devices) {
    if (visible_devices < 1) return 0;
    int64_t g = n / kRowsPerShardAuto;
    if (g < 1) g = 1;
    if (g > visible_devices) g = visible_devices;
    if (g > MI355REC_MAX_SHARDS) g = MI355REC_MAX_SHARDS;
    return static_cast<int>(g);
}

int mi355rec_create_placed(const float* feats_host, int64_t n, int dim, const int* devices, int n_devices, int placement,
                           mi355rec_sharded_t** out) {
    if (out) *out = nullptr;
    if (placement != MI355REC_PLACEMENT_AUTO && placement != MI355REC_PLACEMENT_SHARDED && placement != MI355REC_PLACEMENT_REPLICATED)
        return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "unknown placement %d", placement);
    const int visible = mi355rec_device_count();
    if (visible <= 0) {
        // No device at all.  An explicit device list cannot be honoured; otherwise the catalogue is served by the
        // product's own CPU backend, as the reference falls back to its CPU loop (Recommender.cu:117-127,176-181).
        if (devices || n_devices > 0)
            return sfail(nullptr, MI355REC_ERR_NO_DEVICE, "no HIP device visible, and %d device(s) were asked for", n_devices);
        if (!out || !feats_host) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null argument");
        if (dim != MI355REC_DIM) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "dim must be %d, got %d", MI355REC_DIM, dim);
        if (n < 1 || n > 0xfffffffell) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "rows %lld out of range", (long long)n);
        mi355rec_sharded* h = nullptr;
        try {   // (nothing may leave a C entry point as an exception: the handle and its note allocate)
            h = new mi355rec_sharded();
            h->n = n;
            h->peer_rows = false;
            h->cpu = mi355cpu::node_create(feats_host, n);
            if (!h->cpu) {
                delete h;
                return sfail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "CPU backend: cannot hold %lld rows", (long long)n);
            }
            h->note = "CPU backend: no HIP device visible (" + std::to_string(mi355cpu::threads(mi355cpu::node_catalogue(h->cpu))) +
                      " OpenMP thread(s))";
        } catch (const std::bad_alloc&) {
            if (h && h->cpu) mi355cpu::node_destroy(h->cpu);
            if (h) h->cpu = nullptr;
            delete h;
            return sfail(nullptr, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for the CPU backend's handle");
        }
        *out = h;
        return MI355REC_OK;
    }
    std::vector<int> devs;
    if (devices) {   // an explicit list (a device may repeat: virtual shards / replicas on a one-GPU box)
        if (n_devices < 1 || n_devices > MI355REC_MAX_SHARDS)
            return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "n_devices must be in [1, %d] with an explicit list, got %d", MI355REC_MAX_SHARDS, n_devices);
        devs.assign(devices, devices + n_devices);
    } else {
        if (n_devices < 0 || n_devices > visible)
            return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "n_devices %d but %d device(s) visible", n_devices, visible);
        int g = n_devices;
        if (g == 0)   // the library decides: replicas on every device; shards by the size of the catalogue
            g = placement == MI355REC_PLACEMENT_REPLICATED ? (visible < MI355REC_MAX_SHARDS ? visible : MI355REC_MAX_SHARDS)
                                                            : mi355rec_auto_shards(n, visible);
        devs.resize(g);
        for (int d = 0; d < g; ++d) devs[d] = d;
    }
    return create_on(feats_host, n, dim, devs.data(), static_cast<int>(devs.size()), placement == MI355REC_PLACEMENT_REPLICATED, out);
}

int mi355rec_create_sharded(const float* feats_host, int64_t n, int dim, int n_devices, mi355rec_sharded_t** out) {
    return mi355rec_create_placed(feats_host, n, dim, nullptr, n_devices, MI355REC_PLACEMENT_SHARDED, out);
}

int mi355rec_sharded_placement(const mi355rec_sharded_t* h) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->cpu) return MI355REC_PLACEMENT_CPU;
    return h->replicated ? MI355REC_PLACEMENT_REPLICATED : MI355REC_PLACEMENT_SHARDED;
}

int mi355rec_sharded_set_transport(mi355rec_sharded_t* h, int transport) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->replicated || h->cpu) {   // nothing is ever exchanged (replicas; the CPU backend): either value is accepted and ignored
        if (transport != MI355REC_TRANSPORT_PEER && transport != MI355REC_TRANSPORT_RCCL)
            return sfail(h, MI355REC_ERR_INVALID_ARG, "unknown transport %d", transport);
        return MI355REC_OK;
    }
    if (transport == MI355REC_TRANSPORT_PEER) {
        if (!h->peer_ok) return sfail(h, MI355REC_ERR_INVALID_ARG, "peer access to device %d is not available from every shard", h->shards[0].device);
    } else if (transport != MI355REC_TRANSPORT_RCCL) {
        return sfail(h, MI355REC_ERR_INVALID_ARG, "unknown transport %d", transport);
    }
    if (transport != h->transport) {   // an open stream window is closed under the transport it was filled with
        DeviceRestore restore;
        int rc = stream_flush(h);
        if (rc) return rc;
        rc = drain_workers(h);
        if (rc) return rc;
    }
    h->transport = transport;
    return MI355REC_OK;
}

int mi355rec_sharded_info(const mi355rec_sharded_t* h, int* n_shards, int* transport, int64_t* rows,
                          int* devices_out, int64_t* shard_rows_out) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (n_shards) *n_shards = static_cast<int>(h->shards.size());
    if (transport) *transport = h->transport;
    if (rows) *rows = h->n;
    for (size_t r = 0; r < h->shards.size(); ++r) {
        if (devices_out) devices_out[r] = h->shards[r].device;
        if (shard_rows_out) shard_rows_out[r] = h->shards[r].hi - h->shards[r].lo;
    }
    return MI355REC_OK;
}

const char* mi355rec_sharded_note(const mi355rec_sharded_t* h) { return h ? h->note.c_str() : ""; }

// What RCCL itself says about the communicators of the RCCL transport (include/mi355rec_diag.h): *comms = communicators this
// handle holds (one per shard; 0 until the transport has been used), *ranks = ncclCommCount of the first one, *ranks_agree = 1
// when every communicator reports that same count and its own shard index as its rank.
int mi355rec_sharded_rccl_ranks(const mi355rec_sharded_t* h, int* comms, int* ranks, int* ranks_agree) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    int n_comms = 0, first = 0, agree = 1;
    if (!h->cpu && h->rccl_ready && g_rccl.CommCount) {
        for (size_t r = 0; r < h->shards.size(); ++r) {
            if (!h->shards[r].comm) continue;
            int count = 0, rank = -1;
            if (g_rccl.CommCount(h->shards[r].comm, &count) != 0) count = -1;
            if (g_rccl.CommUserRank && g_rccl.CommUserRank(h->shards[r].comm, &rank) != 0) rank = -1;
            if (n_comms == 0) first = count;
            if (count != first || (g_rccl.CommUserRank && rank != static_cast<int>(r))) agree = 0;
            ++n_comms;
        }
    }
    if (comms) *comms = n_comms;
    if (ranks) *ranks = first;
    if (ranks_agree) *ranks_agree = n_comms > 0 ? agree : 0;
    return MI355REC_OK;
}

int mi355rec_sharded_set_timing(mi355rec_sharded_t* h, int enabled) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->cpu) return MI355REC_OK;   // (no kernels to time)
    const int drc = drain_workers(h);
    if (drc) return drc;
    for (Shard& s : h->shards) S_ENG(h, s, mi355rec_set_timing(s.engine, enabled));
    return MI355REC_OK;
}

int mi355rec_sharded_shard_stats(const mi355rec_sharded_t* hc, int shard, mi355rec_stats_t* out) {
    mi355rec_sharded_t* h = const_cast<mi355rec_sharded_t*>(hc);
    if (!h || !out) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (shard < 0 || shard >= static_cast<int>(h->shards.size()))
        return sfail(h, MI355REC_ERR_INVALID_ARG, h->cpu ? "the CPU backend has no device shard %d" : "no shard %d", shard);
    const int drc = drain_workers(h);
    if (drc) return drc;
    const Shard& s = h->shards[shard];
    S_ENG(h, s, mi355rec_stats(s.engine, out));
    return MI355REC_OK;
}

int mi355rec_sharded_set_replica(mi355rec_sharded_t* h, int mode) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->cpu) return MI355REC_OK;   // (the CPU backend scans the fp32 rows, always)
    DeviceRestore restore;
    int rc = stream_flush(h);
    if (rc) return rc;
    rc = drain_workers(h);
    if (rc) return rc;
    for (Shard& s : h->shards) {
        if (s.hi == s.lo) continue;
        S_ENG(h, s, mi355rec_set_replica(s.engine, mode));
    }
    return MI355REC_OK;
}

int mi355rec_sharded_rows_by_pointer(const mi355rec_sharded_t* h) { return h && h->peer_rows ? 1 : 0; }

int mi355rec_sharded_query_batch_topn(mi355rec_sharded_t* h, const float* queries, int batch,
                                      const int64_t* exclude_global, int topn, int64_t* out_idx, float* out_score,
                                      int* out_count) {
    if (!h || !queries || !out_idx) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (batch < 1) return sfail(h, MI355REC_ERR_INVALID_ARG, "batch must be positive");
    if (topn <= 0) return sfail(h, MI355REC_ERR_INVALID_ARG, "topn must be positive, got %d", topn);
    if (h->cpu) {
        for (int b = 0; b < batch; ++b) {
            const char* why = nullptr;
            const int rc = mi355cpu::node_query(h->cpu, queries + static_cast<size_t>(b) * MI355REC_DIM, exclude_global ? exclude_global[b] : -1,
                                                topn, out_idx + static_cast<size_t>(b) * topn,
                                                out_score ? out_score + static_cast<size_t>(b) * topn : nullptr, out_count ? out_count + b : nullptr, &why);
            if (rc) return cpu_result(h, rc, why);
        }
        return MI355REC_OK;
    }
    if (h->shards.size() == 1) {   // one shard: its own handle is the whole engine (row_base 0)
        const int rc = mi355rec_query_batch_topn(h->shards[0].engine, queries, batch, exclude_global, topn, out_idx, out_score, out_count);
        return rc == MI355REC_OK ? rc : sfail(h, rc, "%s", mi355rec_last_error(h->shards[0].engine));
    }
    if (h->replicated) {   // any replica is the whole engine
        DeviceRestore restore;
        Shard* s = nullptr;
        int rc = take_replica(h, &s);
        if (rc) return rc;
        rc = mi355rec_query_batch_topn(s->engine, queries, batch, exclude_global, topn, out_idx, out_score, out_count);
        return rc == MI355REC_OK ? rc : sfail(h, rc, "replica on device %d: %s", s->device, mi355rec_last_error(s->engine));
    }
    // lists are at most n long
    const int eff = static_cast<int64_t>(topn) < h->n ? topn : static_cast<int>(h->n);
    DeviceRestore restore;
    if (eff > MI355REC_MAX_TOPN_FAST) return run_queries_large(h, queries, exclude_global, batch, eff, topn, out_idx, out_score, out_count);
    const int rc = run_queries(h, queries, nullptr, exclude_global, batch, eff);
    if (rc) return rc;
    copy_rows(h->h_idx, h->h_score, batch, eff, topn, out_idx, out_score, out_count);
    return MI355REC_OK;
}

int mi355rec_sharded_query_topn(mi355rec_sharded_t* h, const float* query12, int64_t exclude_global, int topn,
                                int64_t* out_idx, float* out_score, int* out_count) {
    return mi355rec_sharded_query_batch_topn(h, query12, 1, &exclude_global, topn, out_idx, out_score, out_count);
}

int mi355rec_sharded_query_row_topn(mi355rec_sharded_t* h, int64_t global_row, int topn, int64_t* out_idx,
                                    float* out_score, int* out_count) {
    if (!h || !out_idx) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (global_row < 0 || global_row >= h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)global_row);
    if (topn <= 0) return sfail(h, MI355REC_ERR_INVALID_ARG, "topn must be positive, got %d", topn);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_query(h->cpu, mi355cpu::row(mi355cpu::node_catalogue(h->cpu), global_row), global_row, topn,
                                                  out_idx, out_score, out_count, &why), why);
    }
    if (h->shards.size() == 1) {   // what Recommender::recommendByIndex costs on a one-GPU box: exactly mi355rec_query_row_topn
        const int rc = mi355rec_query_row_topn(h->shards[0].engine, global_row, topn, out_idx, out_score, out_count);
        return rc == MI355REC_OK ? rc : sfail(h, rc, "%s", mi355rec_last_error(h->shards[0].engine));
    }
    if (h->replicated) {
        DeviceRestore restore;
        Shard* s = nullptr;
        int rc = take_replica(h, &s);
        if (rc) return rc;
        rc = mi355rec_query_row_topn(s->engine, global_row, topn, out_idx, out_score, out_count);
        return rc == MI355REC_OK ? rc : sfail(h, rc, "replica on device %d: %s", s->device, mi355rec_last_error(s->engine));
    }
    DeviceRestore restore;
    float q[MI355REC_DIM];
    const float* qptr = nullptr;
    int rc = locate_row(h, global_row, &qptr, q);
    if (rc) return rc;
    const int eff = static_cast<int64_t>(topn) < h->n ? topn : static_cast<int>(h->n);
    if (eff > MI355REC_MAX_TOPN_FAST) {
        if (qptr) {   // cold path: by value
            const Shard* own = owner_of(h, global_row);
            S_ENG(h, *own, mi355rec_fetch_row(own->engine, global_row - own->lo, q));
        }
        return run_queries_large(h, q, &global_row, 1, eff, topn, out_idx, out_score, out_count);
    }
    rc = run_queries(h, q, qptr, &global_row, 1, eff);
    if (rc) return rc;
    copy_rows(h->h_idx, h->h_score, 1, eff, topn, out_idx, out_score, out_count);
    return MI355REC_OK;
}

// ---- LABELS (include/mi355rec_diag.h) ---------------------------------------------------------------------------------
int mi355rec_sharded_set_labels(mi355rec_sharded_t* h, const int32_t* labels_host, int64_t n) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (labels_host && n != h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "%lld labels for a catalogue of %lld rows", (long long)n, (long long)h->n);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_set_labels(h->cpu, labels_host, n, &why), why);
    }
    return set_on_every_shard(h, "labels", [&](mi355rec_t* e, const Shard* s) {
        return s && labels_host ? mi355node::set_group_labels(e, labels_host + s->lo, s->hi - s->lo) : mi355node::set_group_labels(e, nullptr, 0);
    });
}

// ---- GROUP CAPS (include/mi355rec_diag.h) -----------------------------------------------------------------------------
int mi355rec_sharded_set_groups(mi355rec_sharded_t* h, const int32_t* groups_host, int64_t n) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (groups_host && n != h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "%lld groups for a catalogue of %lld rows", (long long)n, (long long)h->n);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_set_groups(h->cpu, groups_host, n, &why), why);
    }
    for (int64_t i = 0; groups_host && i < n; ++i)
        if (groups_host[i] < -1)
            return sfail(h, MI355REC_ERR_INVALID_ARG, "group %d of row %lld: a group id is >= 0, or -1 for no group",
                         static_cast<int>(groups_host[i]), (long long)i);
    if (h->shards.size() > 1 && !h->replicated) {   // row-sharded: the host copy alone
        DeviceRestore restore;
        const int rc = drain_workers(h);
        if (rc) return rc;
        if (!groups_host) {
            h->groups.clear();
            h->has_groups = false;
            return MI355REC_OK;
        }
        try {
            h->groups.assign(groups_host, groups_host + n);   // (the strong guarantee: the previous groups stay)
        } catch (const std::bad_alloc&) {
            return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for the groups (%lld rows)", (long long)n);
        }
        h->has_groups = true;
        return MI355REC_OK;
    }
    return set_on_every_shard(h, "groups", [&](mi355rec_t* e, const Shard* s) {
        return s && groups_host ? mi355node::set_group_groups(e, groups_host + s->lo, s->hi - s->lo) : mi355node::set_group_groups(e, nullptr, 0);
    });
}

// ---- ROW PRIORS (include/mi355rec_diag.h) -----------------------------------------------------------------------------
int mi355rec_sharded_set_priors(mi355rec_sharded_t* h, const float* priors_host, int64_t n) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (priors_host && n != h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "%lld priors for a catalogue of %lld rows", (long long)n, (long long)h->n);
    const int64_t bad = priors_host ? mi355playlist::first_bad_prior(priors_host, n) : -1;
    if (bad >= 0)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "prior %g of row %lld: a prior is finite with |p| <= 1",
                     static_cast<double>(priors_host[bad]), (long long)bad);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_set_priors(h->cpu, priors_host, n, &why), why);
    }
    // every replica the whole array, every shard of a row-sharded placement its slice (each scans its own rows' priors)
    const int rc = set_on_every_shard(h, "priors", [&](mi355rec_t* e, const Shard* s) {
        if (!s) h->has_priors = false;   // (dropped on every shard after one failed)
        return s && priors_host ? mi355node::set_group_priors(e, priors_host + s->lo, s->hi - s->lo) : mi355node::set_group_priors(e, nullptr, 0);
    });
    if (rc == MI355REC_OK) h->has_priors = priors_host != nullptr;
    return rc;
}

namespace {
// A filtered query on a row-sharded catalogue: the query by value on every shard (the query row excluded by its global index).
int sharded_labels_by_value(mi355rec_sharded_t* h, const float* q, int64_t exclude_global, const int32_t* labels, int n_labels,
                            int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return merge_over_shards(h, topn, {out_idx, out_score, nullptr, out_count, nullptr},
                             [&](const Shard& s, const mi355playlist::Outputs& mine) {
                                 return mi355rec_query_topn_labels(s.engine, q, exclude_global, labels, n_labels, topn, mine.idx, mine.score,
                                                                   mine.count);
                             });
}
}  // namespace

int mi355rec_sharded_query_topn_labels(mi355rec_sharded_t* h, const float* query12, int64_t exclude_global, const int32_t* labels,
                                       int n_labels, int topn, int64_t* out_idx, float* out_score, int* out_count) {
    if (!h || !query12 || !out_idx) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (topn <= 0) return sfail(h, MI355REC_ERR_INVALID_ARG, "topn must be positive, got %d", topn);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_query_labels(h->cpu, query12, exclude_global, labels, n_labels, topn, out_idx, out_score,
                                                         out_count, &why), why);
    }
    DeviceRestore restore;
    if (h->shards.size() == 1 || h->replicated)
        return on_whole_catalogue(h, [&](mi355rec_t* e) {
            return mi355rec_query_topn_labels(e, query12, exclude_global, labels, n_labels, topn, out_idx, out_score, out_count);
        });
    const int rc = drain_workers(h);
    if (rc) return rc;
    return sharded_labels_by_value(h, query12, exclude_global, labels, n_labels, topn, out_idx, out_score, out_count);
}

int mi355rec_sharded_query_row_topn_labels(mi355rec_sharded_t* h, int64_t global_row, const int32_t* labels, int n_labels, int topn,
                                           int64_t* out_idx, float* out_score, int* out_count) {
    if (!h || !out_idx) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (global_row < 0 || global_row >= h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)global_row);
    if (topn <= 0) return sfail(h, MI355REC_ERR_INVALID_ARG, "topn must be positive, got %d", topn);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_query_labels(h->cpu, mi355cpu::row(mi355cpu::node_catalogue(h->cpu), global_row), global_row,
                                                         labels, n_labels, topn, out_idx, out_score, out_count, &why), why);
    }
    DeviceRestore restore;
    if (h->shards.size() == 1 || h->replicated)
        return on_whole_catalogue(h, [&](mi355rec_t* e) {
            return mi355rec_query_row_topn_labels(e, global_row, labels, n_labels, topn, out_idx, out_score, out_count);
        });
    const int rc = drain_workers(h);
    if (rc) return rc;
    const Shard* own = owner_of(h, global_row);
    float q[MI355REC_DIM];
    S_HIP(h, hipSetDevice(own->device));
    S_ENG(h, *own, mi355rec_fetch_row(own->engine, global_row - own->lo, q));
    return sharded_labels_by_value(h, q, global_row, labels, n_labels, topn, out_idx, out_score, out_count);
}

// ---- PLAYLISTS, FEATURE FILTERS, WEIGHTED PLAYLISTS, DIVERSIFIED TOP-N, GROUP CAPS (include/mi355rec_diag.h) -----------------
namespace {
using mi355playlist::Outputs;
using mi355playlist::Request;
using mi355playlist::request;

// CANDIDATE LISTS on a ROW-SHARDED catalogue: the request as the shard of rows [lo, hi) takes it, its list cut down to the ids of
// that range (candidates.h); a request without a list as it is.  A shard with none gets an empty list: its call launches nothing,
// as one with nothing left to return.
struct ShardLists {
    std::vector<int64_t> ids;   // the list of the shard asked for last (the shards are asked one after the other)
    Request of(const Request& r, int64_t lo, int64_t hi) {
        if (!r.listed) return r;
        try {
            mi355cand::split(r.candidates, r.n_candidates, lo, hi, &ids);
        } catch (const std::bad_alloc&) {
            return r;   // (the whole list: the shard matches the ids of its own rows itself)
        }
        Request mine = r;
        mine.candidates = ids.data();
        mine.n_candidates = static_cast<int64_t>(ids.size());
        return mine;
    }
};

// The diversified call on a ROW-SHARDED catalogue (members by value, all checked): the pool from every shard's mean call merged
// on the host, its rows gathered from their shards (one mi355rec_fetch_rows per shard that owns any) and the re-rank on the
// first shard's device over the pool passed by value.
int diverse_over_shards(mi355rec_sharded_t* h, const Request& r, const Outputs& out) {
    const int pool = r.pool;
    if (r.capped && !h->has_groups) return sfail(h, MI355REC_ERR_INVALID_ARG, "this handle has no groups (mi355rec_sharded_set_groups)");
    std::vector<int64_t> pidx, local;
    std::vector<float> prel, rows, part;
    std::vector<int> where;
    std::vector<int32_t> pgroups;
    try {
        if (r.capped) pgroups.resize(static_cast<size_t>(pool));
        pidx.resize(static_cast<size_t>(pool));
        prel.resize(static_cast<size_t>(pool));
        rows.resize(static_cast<size_t>(pool) * MI355REC_DIM);
        part.resize(static_cast<size_t>(pool) * MI355REC_DIM);
        local.reserve(static_cast<size_t>(pool));
        where.reserve(static_cast<size_t>(pool));
    } catch (const std::bad_alloc&) {
        return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for a pool of %d rows", pool);
    }
    int p_eff = 0;
    int rc = drain_workers(h);
    if (rc) return rc;
    const Request mean = r.pool_call();
    ShardLists lists;
    rc = merge_over_shards(h, pool, {pidx.data(), prel.data(), nullptr, &p_eff, nullptr},
                           [&](const Shard& s, const Outputs& mine) {
                               return mi355node::query_playlist(s.engine, lists.of(mean, s.lo, s.hi), mine);
                           });
    if (rc) return rc;
    if (p_eff <= 0) {
        mi355playlist::pad(out, 0, r.topn, 0);
        return MI355REC_OK;
    }
    for (Shard& s : h->shards) {
        if (s.hi <= s.lo) continue;
        local.clear();
        where.clear();
        for (int i = 0; i < p_eff; ++i)
            if (pidx[static_cast<size_t>(i)] >= s.lo && pidx[static_cast<size_t>(i)] < s.hi) {
                local.push_back(pidx[static_cast<size_t>(i)] - s.lo);
                where.push_back(i);
            }
        if (local.empty()) continue;
        S_HIP(h, hipSetDevice(s.device));
        S_ENG(h, s, mi355rec_fetch_rows(s.engine, local.data(), static_cast<int64_t>(local.size()), part.data()));
        for (size_t j = 0; j < where.size(); ++j)
            std::memcpy(rows.data() + static_cast<size_t>(where[j]) * MI355REC_DIM, part.data() + j * MI355REC_DIM, sizeof(float) * MI355REC_DIM);
    }
    Shard* first = nullptr;
    for (Shard& s : h->shards)
        if (s.hi > s.lo) {
            first = &s;
            break;
        }
    S_HIP(h, hipSetDevice(first->device));
    for (int i = 0; r.capped && i < p_eff; ++i) pgroups[static_cast<size_t>(i)] = h->groups[static_cast<size_t>(pidx[static_cast<size_t>(i)])];
    S_ENG(h, *first, mi355node::rerank_pool(first->engine, pidx.data(), prel.data(), rows.data(), p_eff, r.lambda, r.topn, out.idx, out.score,
                                            out.mmr, out.count, r.capped ? pgroups.data() : nullptr, r.max_per_group, out.pool_rows));
    return MI355REC_OK;
}

// By row, one handle (row_base 0) takes its own by-row call: the members stay on the device.  Otherwise the members go by value
// (fetched once into `members`) and their rows are added to the exclusion list (`excl`).  r has been checked.
int members_by_value(mi355rec_sharded_t* h, Request& r, float* members, int64_t* excl) {
    if (!(r.rows && (h->cpu || h->shards.size() > 1 || h->replicated))) return MI355REC_OK;
    for (int i = 0; i < r.n_exclude; ++i) excl[i] = r.exclude[i];
    for (int m = 0; m < r.k; ++m) {
        excl[r.n_exclude + m] = r.rows[m];
        if (h->cpu) {
            std::memcpy(members + m * MI355REC_DIM, mi355cpu::row(mi355cpu::node_catalogue(h->cpu), r.rows[m]), sizeof(float) * MI355REC_DIM);
            continue;
        }
        if (m == 0) {
            const int rc = drain_workers(h);
            if (rc) return rc;
        }
        DeviceRestore restore;
        const Shard* own = owner_of(h, r.rows[m]);
        S_HIP(h, hipSetDevice(own->device));
        S_ENG(h, *own, mi355rec_fetch_row(own->engine, r.rows[m] - own->lo, members + m * MI355REC_DIM));
    }
    r.members = members;
    r.rows = nullptr;
    r.exclude = excl;
    r.n_exclude += r.k;
    return MI355REC_OK;
}

// Every call of the family on the node handle: the checks (the catalogue's global rows are known here), the members of a
// by-row call by value where no single handle can read them, then the CPU backend, the one handle that holds the whole
// catalogue, or every shard and a host merge.
int sharded_playlist(mi355rec_sharded_t* h, Request r, const Outputs& out) {
    if (!h || !(r.members || r.rows) || !(out.idx || (r.bounded && r.topn == 0)) || (r.bounded && !out.total))
        return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    char why[128];
    if ((r.diverse && mi355playlist::invalid_diverse(r, why, sizeof why)) ||
        mi355playlist::invalid_playlist(r, h->n, h->n, MI355REC_MAX_EXCLUDE, why, sizeof why))
        return sfail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    if (r.prior && !h->cpu && !h->has_priors)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "this handle has no priors (mi355rec_sharded_set_priors)");
    if (r.rowset && r.rowset->node != h) return sfail(h, MI355REC_ERR_INVALID_ARG, "row set of another handle");
    if (out.pool_rows) *out.pool_rows = 0;
    float members[MI355REC_MAX_PLAYLIST * MI355REC_DIM];
    int64_t excl[MI355REC_MAX_EXCLUDE + MI355REC_MAX_PLAYLIST];
    const int by_value = members_by_value(h, r, members, excl);
    if (by_value) return by_value;
    if (h->cpu) {
        const char* cpu_why = nullptr;
        return cpu_result(h, r.diverse ? mi355cpu::node_query_mean_diverse(h->cpu, r, out, &cpu_why)
                                       : mi355cpu::node_query_mean(h->cpu, r, out, &cpu_why), cpu_why);
    }
    DeviceRestore restore;
    if (h->shards.size() == 1 || h->replicated)
        return on_whole_catalogue(h, [&](mi355rec_t* e) { return mi355node::query_playlist(e, r, out); });
    if (r.diverse) return diverse_over_shards(h, r, out);
    const int rc = drain_workers(h);
    if (rc) return rc;
    // every shard gets the whole exclusion list and matches the ids of its own rows, and its own cut of a candidate list; it
    // answers with its leading keys, each with its member where `out` has members ("ANY-OF REQUESTS"), and its own total where
    // `out` has one ("BOUNDED REQUESTS": the keys are cut at the floor already).  "DISTANCE REQUESTS": the shards answer with -m,
    // what the merge's keys compare; the distances are taken from the merged list.
    const bool report_distance = r.report_distance;
    r.report_distance = false;
    ShardLists lists;
    const int merged = merge_over_shards(h, r.topn, out, [&](const Shard& s, const Outputs& mine) {
        return mi355node::query_playlist(s.engine, lists.of(r, s.lo, s.hi), mine);
    });
    if (merged == MI355REC_OK && report_distance) mi355playlist::scores_to_distances(out, r.topn, r.metric);
    return merged;
}

// CANDIDATE SCORES (include/mi355rec_diag.h) on the node handle: sharded_playlist's checks and member rows, then the CPU backend,
// the one handle that holds the whole catalogue with the whole list, or every shard that owns listed ids with those ids (a shard
// with none launches nothing), its values scattered back to the ids' list positions.  (r.listed and r.score are set; the ids are checked.)
int sharded_scores(mi355rec_sharded_t* h, Request r, const mi355playlist::ScoreOutputs& out) {
    if (!(r.members || r.rows)) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    char why[160];
    if (mi355playlist::invalid_score_request(r, r.n_candidates, out.value, why, sizeof why) ||
        mi355playlist::invalid_playlist(r, h->n, h->n, MI355REC_MAX_EXCLUDE, why, sizeof why))
        return sfail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    if (r.prior && !h->cpu && !h->has_priors)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "this handle has no priors (mi355rec_sharded_set_priors)");
    if (r.rowset && r.rowset->node != h) return sfail(h, MI355REC_ERR_INVALID_ARG, "row set of another handle");
    if (r.n_candidates == 0) return MI355REC_OK;   // nothing to write, nothing to launch
    float members[MI355REC_MAX_PLAYLIST * MI355REC_DIM];
    int64_t excl[MI355REC_MAX_EXCLUDE + MI355REC_MAX_PLAYLIST];
    int rc = members_by_value(h, r, members, excl);
    if (rc) return rc;
    if (h->cpu) {
        const char* cpu_why = nullptr;
        return cpu_result(h, mi355cpu::node_score_rows(h->cpu, r, out, &cpu_why), cpu_why);
    }
    DeviceRestore restore;
    if (h->shards.size() == 1 || h->replicated)
        return on_whole_catalogue(h, [&](mi355rec_t* e) { return mi355node::score_playlist(e, r, out); });
    rc = drain_workers(h);
    if (rc) return rc;
    std::vector<int64_t> ids, where;
    std::vector<float> value;
    std::vector<uint8_t> admissible;
    for (Shard& s : h->shards) {
        if (s.hi <= s.lo) continue;
        try {
            ids.clear();
            where.clear();
            for (int64_t i = 0; i < r.n_candidates; ++i)
                if (r.candidates[i] >= s.lo && r.candidates[i] < s.hi) {
                    ids.push_back(r.candidates[i]);
                    where.push_back(i);
                }
            value.resize(ids.size());
            admissible.resize(ids.size());
        } catch (const std::bad_alloc&) {
            return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for a list of %lld candidates", (long long)r.n_candidates);
        }
        if (ids.empty()) continue;
        Request mine = r;
        mine.candidates = ids.data();
        mine.n_candidates = static_cast<int64_t>(ids.size());
        S_HIP(h, hipSetDevice(s.device));
        S_ENG(h, s, mi355node::score_playlist(s.engine, mine, {value.data(), admissible.data()}));
        for (size_t j = 0; j < where.size(); ++j) {
            out.value[where[j]] = value[j];
            if (out.admissible) out.admissible[where[j]] = admissible[j];
        }
    }
    return MI355REC_OK;
}

// The ONE body of every exported entry point that takes a request struct (playlist_request.h: from_request converts whichever it
// is): the null handle, the conversion, the list's own checks (CANDIDATE LISTS: its ids are rows of the catalogue), then
// sharded_scores with `score`, else sharded_playlist.  (A template: C++ linkage inside this file's extern "C" block.)
extern "C++" template <class Query, class Result>
int node_request_entry(mi355rec_sharded_t* h, const Query* query, const mi355rec_request_ext_t* ext, const Result* result,
                       const mi355playlist::CandidateList& list, const mi355playlist::ScoreOutputs* score = nullptr) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    Query full;
    Request r;
    Outputs out;
    char why[160];
    if (mi355playlist::from_request(query, ext, result, &full, &r, &out, why, sizeof why) ||
        (list.given && mi355cand::invalid_list(list.ids, list.n, MI355REC_MAX_CANDIDATES, h->n, why, sizeof why)))
        return sfail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    r.listed = list.given;
    r.score = score != nullptr;
    r.candidates = list.ids;
    r.n_candidates = list.n;
    return score ? sharded_scores(h, r, *score) : sharded_playlist(h, r, out);
}
}  // namespace

int mi355rec_sharded_query_mean_topn(mi355rec_sharded_t* h, const float* queries, int k, const int64_t* exclude_global, int n_exclude,
                                     int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sharded_playlist(h, request(queries, nullptr, nullptr, k, exclude_global, n_exclude, nullptr, topn),
                            {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_sharded_query_mean_topn_where(mi355rec_sharded_t* h, const float* queries, int k, const int64_t* exclude_global,
                                           int n_exclude, const mi355rec_filter_t* filter, int topn, int64_t* out_idx,
                                           float* out_score, int* out_count) {
    return sharded_playlist(h, request(queries, nullptr, nullptr, k, exclude_global, n_exclude, filter, topn),
                            {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_sharded_query_mean_topn_weighted(mi355rec_sharded_t* h, const float* queries, const float* weights, int k,
                                              const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                              int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sharded_playlist(h, request(queries, nullptr, weights, k, exclude_global, n_exclude, filter, topn),
                            {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_sharded_query_playlist_topn(mi355rec_sharded_t* h, const int64_t* global_rows, int k, const int64_t* exclude_global,
                                         int n_exclude, int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sharded_playlist(h, request(nullptr, global_rows, nullptr, k, exclude_global, n_exclude, nullptr, topn),
                            {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_sharded_query_playlist_topn_where(mi355rec_sharded_t* h, const int64_t* global_rows, int k,
                                               const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                               int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sharded_playlist(h, request(nullptr, global_rows, nullptr, k, exclude_global, n_exclude, filter, topn),
                            {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_sharded_query_playlist_topn_weighted(mi355rec_sharded_t* h, const int64_t* global_rows, const float* weights, int k,
                                                  const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                                  int topn, int64_t* out_idx, float* out_score, int* out_count) {
    return sharded_playlist(h, request(nullptr, global_rows, weights, k, exclude_global, n_exclude, filter, topn),
                            {out_idx, out_score, nullptr, out_count, nullptr});
}

int mi355rec_sharded_query_mean_topn_diverse(mi355rec_sharded_t* h, const float* queries, const float* weights, int k,
                                             const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                             float lambda, int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr,
                                             int* out_count) {
    return sharded_playlist(h, request(queries, nullptr, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool),
                            {out_idx, out_score, out_mmr, out_count, nullptr});
}

int mi355rec_sharded_query_playlist_topn_diverse(mi355rec_sharded_t* h, const int64_t* global_rows, const float* weights, int k,
                                                 const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                                 float lambda, int pool, int topn, int64_t* out_idx, float* out_score, float* out_mmr,
                                                 int* out_count) {
    return sharded_playlist(h, request(nullptr, global_rows, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool),
                            {out_idx, out_score, out_mmr, out_count, nullptr});
}

// GROUP CAPS (include/mi355rec_diag.h): the diversified calls above with the cap; the groups are checked where they live.
int mi355rec_sharded_query_mean_topn_capped(mi355rec_sharded_t* h, const float* queries, const float* weights, int k,
                                             const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                             float lambda, int pool, int max_per_group, int topn, int64_t* out_idx, float* out_score,
                                            float* out_mmr, int* out_count, int* out_pool_rows) {
    return sharded_playlist(
        h, request(queries, nullptr, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool).capped_at(max_per_group),
        {out_idx, out_score, out_mmr, out_count, out_pool_rows});
}

int mi355rec_sharded_query_playlist_topn_capped(mi355rec_sharded_t* h, const int64_t* global_rows, const float* weights, int k,
                                                 const int64_t* exclude_global, int n_exclude, const mi355rec_filter_t* filter,
                                                 float lambda, int pool, int max_per_group, int topn, int64_t* out_idx, float* out_score,
                                                float* out_mmr, int* out_count, int* out_pool_rows) {
    return sharded_playlist(
        h, request(nullptr, global_rows, weights, k, exclude_global, n_exclude, filter, topn).diversified(lambda, pool).capped_at(max_per_group),
        {out_idx, out_score, out_mmr, out_count, out_pool_rows});
}

// PLAYLIST REQUESTS (include/mi355rec_diag.h): the family's one call on the node handle; the label set travels in the Request
// (one handle takes it as it is, a row-sharded catalogue hands it to every shard with that shard's slice of the labels).
// FEATURE SCALES: the scales travel in the Request.  One handle takes it as it is; a row-sharded catalogue has fetched the
// members given by row UNSCALED (sharded_playlist) and forwards them by value with the scales, so every shard's fl(a_j x_j) is
// the by-row value.
// ROW SETS: the set travels in the Request as well (sharded_playlist checks that it is this node's); every shard's scan finds its
// own copy of the bitmap (engine_playlist.hip.h), the CPU backend tests the host bitmap.
int mi355rec_sharded_query_playlist_request_ext(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                const mi355rec_request_ext_t* ext, const mi355rec_playlist_result_t* result) {
    return node_request_entry(h, query, ext, result, {});
}

int mi355rec_sharded_query_playlist_request_scaled(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                   const float* feature_scales, const mi355rec_playlist_result_t* result) {
    const mi355rec_request_ext_t ext = mi355playlist::scales_only_ext(feature_scales);
    return mi355rec_sharded_query_playlist_request_ext(h, query, &ext, result);
}

int mi355rec_sharded_query_playlist_request(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                            const mi355rec_playlist_result_t* result) {
    return mi355rec_sharded_query_playlist_request_ext(h, query, nullptr, result);
}

// DISTANCE REQUESTS (include/mi355rec_diag.h): the same Request with metric = kDistance through sharded_playlist.
int mi355rec_sharded_query_distance_request_ext(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                const mi355rec_request_ext_t* ext, const mi355rec_distance_result_t* result) {
    return node_request_entry(h, query, ext, result, {});
}

int mi355rec_sharded_query_distance_request_scaled(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                   const float* feature_scales, const mi355rec_distance_result_t* result) {
    const mi355rec_request_ext_t ext = mi355playlist::scales_only_ext(feature_scales);
    return mi355rec_sharded_query_distance_request_ext(h, query, &ext, result);
}

int mi355rec_sharded_query_distance_request(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                            const mi355rec_distance_result_t* result) {
    return mi355rec_sharded_query_distance_request_ext(h, query, nullptr, result);
}

// ANY-OF REQUESTS (include/mi355rec_diag.h): the same Request with metric = kAnyOf through sharded_playlist; a row-sharded catalogue
// carries each key's member index through its host merge (merge_over_shards).
int mi355rec_sharded_query_anyof_request(mi355rec_sharded_t* h, const mi355rec_anyof_query_t* query, const mi355rec_request_ext_t* ext,
                                         const mi355rec_anyof_result_t* result) {
    return node_request_entry(h, query, ext, result, {});
}

// MANHATTAN REQUESTS (include/mi355rec_diag.h): the same Request with metric = kManhattan through sharded_playlist, as the distance
// request: the shards answer with -m, what the merge's keys compare, and m is taken from the merged list.
int mi355rec_sharded_query_manhattan_request(mi355rec_sharded_t* h, const mi355rec_manhattan_query_t* query,
                                             const mi355rec_request_ext_t* ext, const mi355rec_manhattan_result_t* result) {
    return node_request_entry(h, query, ext, result, {});
}

// JACCARD REQUESTS (include/mi355rec_diag.h): the same Request with metric = kJaccard through sharded_playlist, as the playlist
// request: the shards answer with v, what the merge's keys compare.
int mi355rec_sharded_query_jaccard_request(mi355rec_sharded_t* h, const mi355rec_jaccard_query_t* query,
                                           const mi355rec_request_ext_t* ext, const mi355rec_jaccard_result_t* result) {
    return node_request_entry(h, query, ext, result, {});
}

// BOUNDED REQUESTS (include/mi355rec_diag.h): the same Request with `bounded` through sharded_playlist; a row-sharded catalogue merges
// the shards' matches and sums their totals (merge_over_shards).
int mi355rec_sharded_query_bounded_request(mi355rec_sharded_t* h, const mi355rec_bounded_query_t* query, const mi355rec_request_ext_t* ext,
                                           const mi355rec_bounded_result_t* result) {
    return node_request_entry(h, query, ext, result, {});
}

// CANDIDATE LISTS (include/mi355rec_diag.h): the list travels in the Request; its ids are rows of the catalogue.  One handle takes it
// whole, a row-sharded catalogue cuts it per shard (ShardLists), the CPU backend searches it.
int mi355rec_sharded_query_playlist_request_candidates(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       const mi355rec_playlist_result_t* result) {
    return node_request_entry(h, query, ext, result, {true, candidates, n_candidates});
}

int mi355rec_sharded_query_distance_request_candidates(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       const mi355rec_distance_result_t* result) {
    return node_request_entry(h, query, ext, result, {true, candidates, n_candidates});
}

// CANDIDATE SCORES (include/mi355rec_diag.h): the _candidates calls' conversion and checks (there is no result struct: an empty one
// stands in), then sharded_scores.
int mi355rec_sharded_score_playlist_request_candidates(mi355rec_sharded_t* h, const mi355rec_playlist_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       float* out_value, uint8_t* out_admissible) {
    const mi355rec_playlist_result_t none = {};
    const mi355playlist::ScoreOutputs score = {out_value, out_admissible};
    return node_request_entry(h, query, ext, &none, {true, candidates, n_candidates}, &score);
}

int mi355rec_sharded_score_distance_request_candidates(mi355rec_sharded_t* h, const mi355rec_distance_query_t* query,
                                                       const mi355rec_request_ext_t* ext, const int64_t* candidates, int64_t n_candidates,
                                                       float* out_distance, uint8_t* out_admissible) {
    const mi355rec_distance_result_t none = {};
    const mi355playlist::ScoreOutputs score = {out_distance, out_admissible};
    return node_request_entry(h, query, ext, &none, {true, candidates, n_candidates}, &score);
}

// ROW SETS (include/mi355rec_diag.h): the global host bitmap, and a device copy beside every engine's rows: a row-sharded placement
// gives each shard the slice [lo, hi) (lo is in general no multiple of 8: rowset.h slices by bit), a replicated one and a single
// shard the whole bitmap.  mi355rec_rowset_add (engine_rowset.hip.h) refreshes every copy.
int mi355rec_sharded_rowset_create(mi355rec_sharded_t* h, const int64_t* global_ids, int64_t n_ids, mi355rec_rowset_t** out) {
    if (!h || !out) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    char why[160];
    if (mi355rowset::invalid_ids(global_ids, n_ids, h->n, why, sizeof why)) return sfail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
    mi355rec_rowset* s = new (std::nothrow) mi355rec_rowset();
    if (!s) return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for a row set");
    s->node = h;
    try {
        s->bits.reset(0, h->n);
    } catch (const std::bad_alloc&) {
        delete s;
        return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for a row set of %lld rows", (long long)h->n);
    }
    s->bits.add(global_ids, n_ids);
    if (!h->cpu) {
        DeviceRestore restore;
        for (Shard& sh : h->shards) {
            if (sh.hi <= sh.lo) continue;
            const int rc = mi355node::rowset_attach(s, sh.engine, sh.lo, sh.hi, why, sizeof why);
            if (rc != MI355REC_OK) {
                mi355rec_rowset_destroy(s);
                return sfail(h, rc, "shard on device %d: %s", sh.device, why);
            }
        }
    }
    *out = s;
    return MI355REC_OK;
}

// ROW UPDATES (include/mi355rec_diag.h): the node handle owns its rows, so an update always brings them.  The open window is closed
// and the workers are drained first (tickets already waited for stay readable: their results are in host memory); then the
// caller's thread drives the engines itself.  Row-sharded: every shard gets the rows it owns, made local.  Replicated: every
// device once — a replica on a device that already holds one is a lane of it and shares its rows and replicas.
int mi355rec_sharded_update_rows(mi355rec_sharded_t* h, const int64_t* global_rows, int64_t count, const float* feats_host) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (count < 0 || (count > 0 && !global_rows)) return sfail(h, MI355REC_ERR_INVALID_ARG, "null rows / negative count");
    if (count == 0) return MI355REC_OK;
    if (!feats_host) return sfail(h, MI355REC_ERR_INVALID_ARG, "a node handle owns its rows: an update brings them (feats_host is NULL)");
    std::vector<mi355update::ShardPart> parts;
    std::vector<float> rows;
    try {
        int64_t at = 0;
        const mi355update::Bad bad = mi355update::check_rows(global_rows, count, h->n, &at);
        if (bad != mi355update::kFine) {
            char why[160];
            mi355update::describe(bad, global_rows, at, h->n, why, sizeof why);
            return sfail(h, MI355REC_ERR_INVALID_ARG, "%s", why);
        }
        if (!h->cpu && !h->replicated && h->shards.size() > 1) {
            std::vector<int64_t> lo(h->shards.size());
            for (size_t r = 0; r < h->shards.size(); ++r) lo[r] = h->shards[r].lo;
            mi355update::split_by_shard(global_rows, count, lo.data(), static_cast<int>(lo.size()), parts);
        }
    } catch (const std::bad_alloc&) {
        return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for an update of %lld rows", (long long)count);
    }
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_update_rows(h->cpu, global_rows, count, feats_host, &why), why);
    }
    DeviceRestore restore;
    // (the workers have only ENQUEUED the window's scans: every shard's stream is drained before a row is written, as ensure_stream
    // does before it replaces the stream's buffers — the engines wait for their lanes' streams again themselves)
    const int rc = quiesce(h);
    if (rc) return rc;
    // A failure on one shard leaves the shards before it updated: the update may have been applied in part, and repeating it
    // (the same rows, the same features) is safe.
    for (size_t r = 0; r < h->shards.size(); ++r) {
        Shard& s = h->shards[r];
        if (s.hi == s.lo) continue;
        S_HIP(h, hipSetDevice(s.device));
        if (parts.empty()) {   // one shard, or replicas: the whole list, once per device
            if (s.lane) continue;
            S_ENG(h, s, mi355rec_update_rows(s.engine, global_rows, count, feats_host));
            continue;
        }
        const mi355update::ShardPart& part = parts[r];
        if (part.local.empty()) continue;
        try {
            rows.resize(part.local.size() * MI355REC_DIM);
        } catch (const std::bad_alloc&) {
            return sfail(h, MI355REC_ERR_OUT_OF_MEMORY, "out of host memory for an update of %lld rows", (long long)count);
        }
        for (size_t i = 0; i < part.at.size(); ++i)
            std::memcpy(&rows[i * MI355REC_DIM], feats_host + static_cast<size_t>(part.at[i]) * MI355REC_DIM, sizeof(float) * MI355REC_DIM);
        S_ENG(h, s, mi355rec_update_rows(s.engine, part.local.data(), static_cast<int64_t>(part.local.size()), rows.data()));
    }
    return MI355REC_OK;
}

// What a node handle is made of (include/mi355rec_diag.h): host-only accessors for a companion library.
int mi355rec_sharded_shard_handle(mi355rec_sharded_t* h, int shard, mi355rec_t** out) {
    if (!h || !out) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (shard < 0 || shard >= static_cast<int>(h->shards.size()))
        return sfail(h, MI355REC_ERR_INVALID_ARG, h->cpu ? "the CPU backend has no device shard %d" : "no shard %d", shard);
    const int drc = drain_workers(h);
    if (drc) return drc;
    *out = h->shards[shard].engine;
    return MI355REC_OK;
}

int mi355rec_sharded_host_rows(const mi355rec_sharded_t* hc, const float** rows, int64_t* n) {
    mi355rec_sharded_t* h = const_cast<mi355rec_sharded_t*>(hc);
    if (!h || !rows || !n) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (!h->cpu) return sfail(h, MI355REC_ERR_INVALID_ARG, "only the CPU placement keeps its rows on the host");
    const mi355cpu::Catalogue* c = mi355cpu::node_catalogue(h->cpu);
    *n = mi355cpu::rows(c);
    *rows = *n > 0 ? mi355cpu::row(c, 0) : nullptr;
    return MI355REC_OK;
}

int mi355rec_sharded_scores_row(mi355rec_sharded_t* h, int64_t global_row, float* out_host) {
    if (!h || !out_host) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (global_row < 0 || global_row >= h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)global_row);
    if (h->cpu) {
        const mi355cpu::Catalogue* c = mi355cpu::node_catalogue(h->cpu);
        mi355cpu::scores(c, mi355cpu::row(c, global_row), out_host);
        return MI355REC_OK;
    }
    DeviceRestore restore;
    if (h->replicated) {
        Shard* s = nullptr;
        int rc = take_replica(h, &s);
        if (rc) return rc;
        rc = mi355rec_scores_row(s->engine, global_row, out_host);
        return rc == MI355REC_OK ? rc : sfail(h, rc, "replica on device %d: %s", s->device, mi355rec_last_error(s->engine));
    }
    float q[MI355REC_DIM];
    const Shard* own = owner_of(h, global_row);
    int rc = drain_workers(h);   // cold path: the caller's thread drives every shard itself
    if (rc) return rc;
    S_ENG(h, *own, mi355rec_fetch_row(own->engine, global_row - own->lo, q));
    for (const Shard& s : h->shards) {
        if (s.hi == s.lo) continue;
        S_ENG(h, s, mi355rec_scores(s.engine, q, out_host + s.lo));
    }
    return MI355REC_OK;
}

// ---- the stream ---------------------------------------------------------------------------

int mi355rec_sharded_set_window(mi355rec_sharded_t* h, int window) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (window < 1 || window > kMaxWindow) return sfail(h, MI355REC_ERR_INVALID_ARG, "window must be in [1, %d], got %d", kMaxWindow, window);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_set_window(h->cpu, window, &why), why);
    }
    if (window == h->s_window) return MI355REC_OK;
    DeviceRestore restore;
    const int rc = quiesce(h);   // the open window is closed in the old geometry
    if (rc) return rc;
    // buffers are re-made by the next enqueue (ensure_stream sees s_alloc_window != s_window); tickets keep growing, aligned to
    // the NEW window before s_window changes
    h->next_ticket = (h->next_ticket + window - 1) / window * window;
    h->issued_upto = h->next_ticket;
    reset_stream(h);
    h->s_window = window;
    return MI355REC_OK;
}

int mi355rec_sharded_set_window_mode(mi355rec_sharded_t* h, int batched) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->cpu) return MI355REC_OK;   // (a query is computed when it is enqueued, either way)
    if ((batched != 0) == h->batched_windows) return MI355REC_OK;
    DeviceRestore restore;
    const int rc = quiesce(h);
    if (rc) return rc;
    reset_stream(h);   // the next enqueue re-makes the buffers and decides the mode again
    h->batched_windows = batched != 0;
    return MI355REC_OK;
}

int mi355rec_sharded_enqueue_query(mi355rec_sharded_t* h, const float* query12, int64_t exclude_global, int topn,
                                   int64_t* ticket) {
    if (!h || !query12) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_enqueue(h->cpu, query12, exclude_global, topn, ticket, &why), why);
    }
    DeviceRestore restore;
    return stream_enqueue(h, nullptr, query12, exclude_global, topn, ticket);
}

int mi355rec_sharded_enqueue_row(mi355rec_sharded_t* h, int64_t global_row, int topn, int64_t* ticket) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (global_row < 0 || global_row >= h->n)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "Invalid song index: %lld", (long long)global_row);
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_enqueue(h->cpu, mi355cpu::row(mi355cpu::node_catalogue(h->cpu), global_row), global_row, topn,
                                                    ticket, &why), why);
    }
    DeviceRestore restore;
    float q[MI355REC_DIM] = {0};
    const float* qptr = nullptr;
    if (!h->replicated) {
        const int rc = locate_row(h, global_row, &qptr, q);
        if (rc) return rc;
    }
    return stream_enqueue(h, qptr, q, global_row, topn, ticket, global_row);
}

int mi355rec_sharded_enqueue_flush(mi355rec_sharded_t* h) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->cpu) return mi355cpu::node_flush(h->cpu);
    DeviceRestore restore;
    const int64_t t0 = now_ns();
    const int rc = stream_flush(h);
    h->st_host_ns += now_ns() - t0;
    return rc;
}

int mi355rec_sharded_wait(mi355rec_sharded_t* h, int64_t ticket, int64_t* out_idx, float* out_score, int* out_count) {
    if (!h || !out_idx) return sfail(h, MI355REC_ERR_INVALID_ARG, "null argument");
    if (h->cpu) {
        const char* why = nullptr;
        return cpu_result(h, mi355cpu::node_wait(h->cpu, ticket, out_idx, out_score, out_count, &why), why);
    }
    if (!h->s_topn || ticket < 0 || ticket >= h->next_ticket)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "ticket %lld was never handed out", (long long)ticket);
    DeviceRestore restore;
    const int W = h->s_window;
    const int64_t abs = ticket / W;
    const int w = static_cast<int>(abs % kStreamDepth);
    const int slot = static_cast<int>(ticket % W);
    Window& win = h->win[w];
    if (win.abs != abs || slot >= win.count)
        return sfail(h, MI355REC_ERR_INVALID_ARG, "the results of ticket %lld are no longer kept (ring of %d windows of %d)",
                     (long long)ticket, kStreamDepth, W);
    if (!win.issued) {   // its window is still open (or waits for the lag): close it now
        const int rc = stream_flush(h);
        if (rc) return rc;
    }
    {
        const int rc = wait_window(h, w);   // the merge has been enqueued, `merged` recorded, and the results are in host memory
        if (rc) return rc;
    }
    const int topn = h->s_topn;
    const size_t off = (static_cast<size_t>(w) * W + slot) * topn;
    copy_rows(h->s_hidx + off, h->s_hscore + off, 1, topn, topn, out_idx, out_score, out_count);
    return MI355REC_OK;
}

int mi355rec_sharded_stream_stats(const mi355rec_sharded_t* h, int64_t* queries, int64_t* exchanges, int64_t* host_ns) {
    if (!h) return sfail(nullptr, MI355REC_ERR_INVALID_ARG, "null handle");
    if (h->cpu) {
        mi355cpu::node_stream_stats(h->cpu, queries, exchanges, host_ns);   // ("exchanges": windows opened)
        return MI355REC_OK;
    }
    if (queries) *queries = h->st_queries;
    if (exchanges) *exchanges = h->st_exchanges;
    if (host_ns) *host_ns = h->st_host_ns;
    return MI355REC_OK;
}

}  // extern "C"
