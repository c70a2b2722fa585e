// engine_single.hip.h — ONE query at a time: which rows its scan streams (fp32, 8-bit replica), the sample / neighbourhood
// launch in front of a query alone, the scan + merge (replaces calculateSimilarities + the host heap, Recommender.cu:184-254,
// 293-315), rounds for topn > 1024, the completion word of a synchronous query, and the STREAM of single queries that runs
// one call behind so that every launch carries the next query's seed riders — or, where two queued queries share one pass
// over the 8-bit replica ("pairs"), up to three, and up to seven where two pairs share one launch ("groups").  (Part of
// mi355rec.hip's translation unit.)
#pragma once

#include "engine_state.hip.h"

#include <type_traits>

namespace {

int flush_mstream(mi355rec* h, hipStream_t s);   // (engine_batch.hip.h: a stream of BATCHES on the handle is closed before a single query joins)

bool use_half(const mi355rec* h, const uint64_t* upper_dev) {
    if (!h->d_half || upper_dev || h->replica_mode == MI355REC_REPLICA_OFF) return false;
    return h->replica_mode == MI355REC_REPLICA_ON || h->replica_mode == MI355REC_REPLICA_FP16 || h->n >= kHalfAutoMinRows;
}

// Single queries stream the 8-bit replica (half the fp16 one's bytes per row); experiment builds can keep them on the
// fp16 one (MI355REC_REPLICA_FP16: A/B).
bool use_q8(const mi355rec* h) { return h->d_q8 && h->replica_mode != MI355REC_REPLICA_FP16; }

// Which rows the next single query on this handle streams.
int single_kind(const mi355rec* h, const uint64_t* upper_dev) {
    if (!use_half(h, upper_dev)) return kFp32;
    return use_q8(h) ? kQ8 : kFp16;
}

// The sample holds EXACT scores of its rows (one margin in the cutoff instead of two: a third of the candidates)
// where the extra fetch per sampled wave is not on the launch's critical path.
bool q8_exact_sample(const mi355rec* h) { return h->geom[kQ8].iters >= 3; }

// Which sample the next query over `kind` rows takes (mi355rec_set_sample): the bucketed one (replica_q8.hip.h) where the handle
// has the structure and was told to, or — AUTO — for topn <= 128 on shards of MI355REC_SAMPLE_AUTO_MIN_ROWS rows and more
// where the sample is CARRIED by the riders of the launch before.  (Only top-10 and top-100 were modelled: 1024 values of
// which the topn-th is wanted.  A sample launch of its own — a query alone, the first of a stream — is on the query's critical
// path, and there the strided sample's one round trip in 256 workgroups beats the bucketed one's chain of four in eight:
// 5.4 against 14.3 us, 42.0 against 48.4 us for a lone query at 10 M rows.)
constexpr int kBucketAutoMaxTopn = 128;
bool use_bucket(const mi355rec* h, int kind, int topn, bool carried) {
    if (kind != kQ8 || !h->bsample.rows || !q8_exact_sample(h) || h->sample_mode == MI355REC_SAMPLE_STRIDED) return false;
    if (h->sample_mode == MI355REC_SAMPLE_BUCKETED) return true;
    return carried && topn <= kBucketAutoMaxTopn && h->n >= MI355REC_SAMPLE_AUTO_MIN_ROWS;
}
BucketSample bucket_arg(const mi355rec* h) {
    const BucketBufs& b = h->bsample;
    BucketSample bs;
    std::memset(&bs, 0, sizeof bs);
    bs.q8 = static_cast<const uint4*>(b.q8);
    bs.rows = b.rows;
    bs.centroids = b.centroids;
    bs.region_tab = reinterpret_cast<const int2*>(b.region_tab);
    bs.regions = b.regions;
    bs.n_centroids = b.n_centroids;
    bs.picks = b.regions < kBucketPicks ? b.regions : kBucketPicks;
    return bs;
}
// The geometry of a streamed launch over `kind` rows whose riders take the next query's sample, bucketed or not.
const ScanGeom& stream_geom(const mi355rec* h, int kind, bool next_bucketed) { return next_bucketed ? h->geom_bucket : h->geom[kind]; }
// How many sample values a scan over the 8-bit replica selects from, negative where they are exact scores (scan_q8_kernel).
int q8_seed_count(const mi355rec* h, bool bucketed) {
    if (bucketed) return -(kBucketPicks * kBucketGroups);
    const int n_seed = h->geom[kQ8].seed_grid * kHalfSeedWaves;
    return q8_exact_sample(h) ? -n_seed : n_seed;
}

// Does a neighbourhood give the scan a bound (handoff.hip.h)?  Around the row the query excludes when that is a row of THIS
// shard, else (a query by value, a row of another shard) around the query's anchor — on every shard large enough to have one.
bool nbhd_applies(const mi355rec* h, int64_t exclude_global) {
    (void)exclude_global;
    return h->n >= kNbhdRows;
}

// Every kernel that takes a query exists twice: kQueryFromRow reads the 12 floats from `qptr` (a resident row, or any
// other device-readable address), the other takes them by value in its QueryArg / NextSeed and is handed kNoQueryPtr.
// fn(std::true_type or std::false_type, the pointer argument) launches the one that serves this query.
template <typename Fn>
void by_query_form(const float* qptr, Fn&& fn) {
    if (qptr) fn(std::true_type(), qptr);
    else fn(std::false_type(), kNoQueryPtr);
}

// ---- the arguments every scan launch is assembled from --------------------------------------------------------------
QueryArg make_query_arg(const mi355rec* h, const float* qptr, const float* query12) {
    QueryArg qa;
    std::memset(&qa, 0, sizeof qa);
    qa.margin = h->margin_mix;
    if (!qptr) std::memcpy(qa.q, query12, sizeof qa.q);
    return qa;
}

// A launch with no merge of a query before riding in it, none of its own lists at its tail, nothing for a query after.
PrevMerge no_prev_merge() { return PrevMerge{nullptr, 0, 0, nullptr}; }
LoneTail no_lone_tail() { return LoneTail{nullptr, nullptr, nullptr, nullptr, nullptr, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}; }
NextSeed no_next_seed() {
    NextSeed sd;
    std::memset(&sd, 0, sizeof sd);
    return sd;
}

// What a launch takes for the query AFTER the one it scans for (handoff.hip.h) — or, in a sample launch of its own,
// for the query itself: `wgs` workgroups sample the regions of `kind` rows into `out` and (`nbhd`) one more takes the
// query's neighbourhood.  ctl != null: the last of the `wgs` to arrive leaves the bound there; its arrival counter
// counts up from `ctl_done` and is never reset.  The test hooks of mi355rec_debug_handoff apply to ONE sampling
// launch: this one.
NextSeed make_next_seed(mi355rec* h, int kind, int wgs, bool nbhd, const float* qptr, const float* query12, int64_t exclude_global,
                        int topn, uint32_t epoch, unsigned long long* out, SeedCtl* ctl, unsigned ctl_done, bool bucketed = false) {
    const ScanGeom& g = h->geom[kind];
    NextSeed sd = no_next_seed();
    sd.anchors = h->d_anchor;
    sd.query_ptr = qptr;
    if (!qptr) std::memcpy(sd.q, query12, sizeof sd.q);
    sd.exclude_global = exclude_global;
    sd.out = out;
    sd.n_wgs = wgs;
    sd.nbhd = nbhd ? 1 : 0;   // (it stores its slot even when the excluded row is not of this shard)
    sd.regions = g.seed_grid;
    sd.stride_rows = g.seed_stride;
    sd.ctl = wgs > 0 ? ctl : nullptr;
    sd.topk = topn;
    sd.exact = kind == kQ8 && q8_exact_sample(h);
    if (bucketed) sd.bucket = bucket_arg(h);   // (its values are exact scores: use_bucket)
    sd.epoch = epoch;
    if (sd.ctl) sd.done_base = ctl_done + (h->dbg_no_last ? 0x40000000u : 0u);
    sd.debug_skip = h->dbg_skip_regions;
    h->dbg_no_last = false;
    h->dbg_skip_regions = 0;
    return sd;
}

// The sample launch of a query ALONE over a replica (the first query of a stream as well): the sampled regions and,
// when the excluded row is a row of this shard, one more workgroup for its neighbourhood.  The values are tagged with
// `epoch`, which the scan that reads them is given as well.
void enqueue_half_seed(mi355rec* h, int kind, const float* qptr, const float* query12, int64_t exclude_global, int topn,
                       unsigned long long* seed_buf, uint32_t epoch, hipStream_t s, bool bucketed = false) {
    const ScanGeom& g = h->geom[kind];
    const QueryArg qa = make_query_arg(h, qptr, query12);
    if (kind == kQ8) {
        const int extra = nbhd_applies(h, exclude_global) ? 1 : 0;
        BucketSample bs;
        std::memset(&bs, 0, sizeof bs);
        int wgs = g.seed_grid;
        if (bucketed) {   // a handful of workgroups share its regions, kBucketAhead each per round trip
            bs = bucket_arg(h);
            wgs = (bs.picks + kBucketAhead - 1) / kBucketAhead;
        }
        if (wgs + extra <= 0) return;
        hipLaunchKernelGGL(seed_q8_kernel, dim3(wgs + extra), dim3(kHalfSeedBlock), 0, s, h->d_feats, h->d_q8, h->n,
                           g.seed_stride, h->row_base, qa, qptr, exclude_global, seed_buf, epoch, wgs, topn,
                           static_cast<const float*>(h->d_anchor), q8_exact_sample(h), bs);
        return;
    }
#ifdef MI355REC_EXPERIMENTS
    if (g.seed_grid <= 0) return;
    by_query_form(qptr, [&](auto from_row, const float* qp) {
        hipLaunchKernelGGL((seed_half_kernel<decltype(from_row)::value>), dim3(g.seed_grid), dim3(kHalfSeedBlock), 0, s, h->d_feats,
                           h->d_half, h->n, g.seed_stride, h->row_base, qa, qp, exclude_global,
                           reinterpret_cast<uint32_t*>(seed_buf));   // (the fp16 scan's plain values)
    });
#endif
}

// The same for a query alone over the fp32 rows (kernels.hip.h, seed_f32_kernel): one workgroup per region, the last
// to arrive leaves the bound in `ctl`, the neighbourhood workgroup its own in seed_buf[kNbhdSlot].  `*ctl_done` is what
// ctl->done holds (the counter is never reset).  Returns whether a sample (hence a bound in `ctl`) was enqueued.
bool enqueue_f32_seed(mi355rec* h, const float* qptr, const float* query12, int64_t exclude_global, int topn,
                      unsigned long long* seed_buf, SeedCtl* ctl, unsigned* ctl_done, uint32_t epoch, hipStream_t s) {
    const int regions = h->geom[kFp32].seed_grid;
    const int nbhd = nbhd_applies(h, exclude_global) ? 1 : 0;
    if (regions + nbhd <= 0) return false;
    const NextSeed sd = make_next_seed(h, kFp32, regions, nbhd != 0, qptr, query12, exclude_global, topn, epoch, seed_buf, ctl, *ctl_done);
    hipLaunchKernelGGL(seed_f32_kernel, dim3(regions + nbhd), dim3(kHalfSeedBlock), 0, s, h->d_feats, h->n, h->row_base, sd);
    *ctl_done += static_cast<unsigned>(regions);
    return regions > 0;
}

// ---- one scan launch ------------------------------------------------------------------------------------------------
// What the launch of a query alone, its lone-fused form and the launch of a streamed query differ in; the rest is the
// kind's own (launch_scan).
struct ScanLaunch {
    int kind = kFp32;                           // which rows it streams
    bool bucketed = false;                      // 8-bit replica: the query's sample is the bucketed one (what `sample` holds)
    bool streamed = false;                      // one workgroup behind the scanners merges `prev`, and `next` may ask for more
    int grid = 0;                               // workgroups in all ...
    int iters = 0;                              // ... and the tiles of a scanning one
    uint64_t* lists = nullptr;                  // one list per scanning workgroup
    unsigned long long* sample = nullptr;       // the query's sample values (null: fp32 rows without a sample) ...
    const unsigned long long* bound = nullptr;  // ... the launch-wide bound, where somebody has made one of them already ...
    uint32_t epoch = 0u;                        // ... and the tag of both
    const uint64_t* upper = nullptr;            // fp32 rows: a later round of topn > 1024 keeps keys below this one
    PrevMerge prev = no_prev_merge();
    NextSeed next = no_next_seed();
    LoneTail tail = no_lone_tail();             // 8-bit replica, counters != null: the launch merges its own lists (merge.hip.h, lone_tail)
};

// Launches it and, once the launch is known to have been accepted, moves the books: a refused launch leaves host and
// device counters in step.
int launch_scan(mi355rec* h, const ScanLaunch& L, const float* qptr, const float* query12, int64_t exclude_global, int topn,
                hipStream_t s) {
    const QueryArg qa = make_query_arg(h, qptr, query12);
    const dim3 grid(static_cast<unsigned>(L.grid));
    const bool fused = L.tail.counters != nullptr;
    if (L.kind == kQ8) {
        const int q8_seeds = q8_seed_count(h, L.bucketed);   // (negative: exact values)
        by_query_form(qptr, [&](auto from_row, const float* qp) {
            constexpr bool kRow = decltype(from_row)::value;
            auto launch = [&](auto kernel) {
                LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, kernel, grid, dim3(Q8Config::kBlock), s,
                             h->d_feats, h->d_q8, h->n, L.iters, h->row_base, qa, qp, exclude_global, topn, L.lists, L.sample,
                             q8_seeds, h->d_half_rescored, L.prev, L.next, L.bound, L.tail, L.epoch);
            };
            if (L.streamed) launch(scan_q8_kernel<Q8Config, false, true>);   // (one streamed form: it tests qp at run time)
            else if (fused) launch(scan_q8_kernel<Q8Config, kRow, false, true>);
            else launch(scan_q8_kernel<Q8Config, kRow, false>);
        });
#ifdef MI355REC_EXPERIMENTS
    } else if (L.kind == kFp16) {
        const int n_seed = h->geom[kFp16].seed_grid * kHalfSeedWaves;
        by_query_form(qptr, [&](auto from_row, const float* qp) {
            constexpr bool kRow = decltype(from_row)::value;
            auto launch = [&](auto kernel) {
                LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, kernel, grid, dim3(HalfConfig::kBlock), s,
                             h->d_feats, h->d_half, h->n, L.iters, h->row_base, qa, qp, exclude_global, topn, L.lists,
                             reinterpret_cast<uint32_t*>(L.sample), n_seed, h->d_half_rescored, L.prev, L.next);   // (plain sample values)
            };
            if (L.streamed) launch(scan_half_kernel<HalfConfig, kRow, true>);
            else launch(scan_half_kernel<HalfConfig, kRow, false>);
        });
#endif
    } else {
        by_query_form(qptr, [&](auto from_row, const float* qp) {
            constexpr bool kRow = decltype(from_row)::value;
            auto launch = [&](auto kernel) {   // (rows_per_block = 0: tiles dealt round-robin)
                LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, kernel, grid, dim3(kScanBlock), s,
                             h->d_feats, h->n, static_cast<int64_t>(0), L.iters, h->row_base, qa, qp, exclude_global, topn, L.lists,
                             static_cast<float*>(nullptr), L.upper, L.prev, L.bound, L.sample, L.epoch, L.next);
            };
            if (L.streamed) launch(scan_kernel<ScanConfig, kRow, false, 0, true>);
            else launch(scan_kernel<ScanConfig, kRow, false>);
        });
    }
    HIP_TRY(h, hipGetLastError());
    if (L.kind == kFp32) {
        ++h->routes.fp32;
        return MI355REC_OK;
    }
    ++h->half_scans;
    if (L.kind == kFp16) {
        ++h->routes.fp16;
        return MI355REC_OK;
    }
    ++h->q8_scans;
    ++(fused ? h->routes.q8_lone : h->routes.q8);
    if (fused) {   // the arrival counters of the launch's tail count up and are never reset
        for (unsigned g = 0; g < 8u; ++g) h->lone_base[g] += lone_tail_members(grid.x, g);
        h->lone_base[8] += lone_tail_groups(grid.x);
    }
    return MI355REC_OK;
}

// Enqueue the scan for one query.  qptr != null: the kernel reads the query's 12 floats from there
// (a resident row, or any other device-readable address).
// *n_lists = per-workgroup lists it leaves in d_block_lists.
// lone != null (a lone query whose caller waits on the host): over the 8-bit replica of a large shard the launch
// also merges its own lists into lone's buffers (merge.hip.h, lone_tail) and *fused is set.
constexpr int64_t kLoneFusedMinRows = 4000000;
// A query alone over the fp32 rows gets a sample launch of its own (~5 us) from here up: below, the scan is a dozen
// microseconds and launch-bound.
constexpr int64_t kF32LoneSeedMinRows = 4000000;
// (Round 4 had a LONE synchronous query below 1.5 M rows read the fp32 rows — two launches against the replica's three
// were worth more than the bytes: 27.3 against 29.7 us at 1 M rows.  Once the 8-bit scan's prologue had been fixed —
// sample requested before the first tile, one LDS atomic per wave in its selection — the replica won from 1 M rows up
// again (tools/route_thresholds.sh: 25.7 against 27.4 us at 1 M, 27.1 against 30.4 at 1.4 M, 28.3 against 39.9 at 3 M;
// 28.0 against 24.3 at 0.7 M), which is where single queries take it anyway: the rule is gone.)
int enqueue_scan(mi355rec* h, const float* qptr, const float* query12,
                 int64_t exclude_global, int topn, const uint64_t* upper_dev, hipStream_t s, int* n_lists,
                 const LoneTail* lone = nullptr, bool* fused = nullptr) {
    if (fused) *fused = false;
    ScanLaunch L;
    L.kind = single_kind(h, upper_dev);
    L.grid = *n_lists = h->geom[L.kind].grid;
    L.iters = h->geom[L.kind].iters;
    L.lists = h->d_block_lists;
    L.upper = upper_dev;
    if (L.kind != kFp32) {
        if (L.kind == kQ8) L.epoch = next_epoch(h);
        L.sample = h->d_half_seed;
        L.bucketed = use_bucket(h, L.kind, topn, false);
        if (L.kind == kQ8) h->last_sample = L.bucketed ? MI355REC_SAMPLE_BUCKETED : MI355REC_SAMPLE_STRIDED;
        enqueue_half_seed(h, L.kind, qptr, query12, exclude_global, topn, h->d_half_seed, L.epoch, s, L.bucketed);
        if (L.kind == kQ8 && lone && h->n >= kLoneFusedMinRows) {
            L.tail = *lone;   // ... whose arrival counters start this launch from
            for (unsigned g = 0; g < 9u; ++g) L.tail.base[g] = h->lone_base[g];
        }
    } else if (!upper_dev && h->n >= kF32LoneSeedMinRows) {
        // The launch-wide bound (kernels.hip.h): on shards where ~5 us are worth it, and never for the later rounds of
        // topn > 1024 (they look for keys BELOW the round before: a lower bound on the best keys says nothing there).
        L.epoch = next_epoch(h);
        if (enqueue_f32_seed(h, qptr, query12, exclude_global, topn, h->d_half_seed, h->d_lone_ctl, &h->lone_ctl_done, L.epoch, s))
            L.bound = &h->d_lone_ctl->cutoff;
        L.sample = h->d_half_seed;
    }
    const int rc = launch_scan(h, L, qptr, query12, exclude_global, topn, s);
    if (rc == MI355REC_OK && fused) *fused = L.tail.counters != nullptr;
    return rc;
}

int enqueue_merge(mi355rec* h, const uint64_t* lists, int n_lists, int list_len, int topn,
                  uint64_t* out_keys, int64_t* out_idx, float* out_score, hipStream_t s, uint32_t notify = 0) {
    const int slot = timing_begin(h, h->ev_merge, h->n_merge_pairs, h->merge_launches, s);
    // notify: the host polls h->h_done for this value (mi355rec_query_row_topn); 0: no completion word
    hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kMergeBlock), 0, s, lists, n_lists, list_len,
                       static_cast<int64_t>(list_len), static_cast<int64_t>(0), topn, out_keys, out_idx, out_score,
                       static_cast<int64_t>(0), notify ? h->hd_done : static_cast<uint32_t*>(nullptr), notify);
    timing_end(h, h->ev_merge, h->n_merge_pairs, slot, s);
    HIP_TRY(h, hipGetLastError());
    return MI355REC_OK;
}

int check_topn(mi355rec* h, int topn, bool allow_rounds) {
    if (topn <= 0)
        return fail(h, MI355REC_ERR_INVALID_ARG, "topn must be positive, got %d", topn);
    if (!allow_rounds && topn > kMaxTopK)
        return fail(h, MI355REC_ERR_INVALID_ARG, "topn %d > %d is not supported by this call", topn, kMaxTopK);
    return MI355REC_OK;
}

// One query end to end on stream `s`: scan + merge, in rounds of kMaxTopK when
// topn is larger (round r only sees keys below the last key of round r-1, read
// from device memory, so the rounds are enqueued back to back without a sync).
bool pairs_open(const mi355rec* h);
int flush_streamed(mi355rec* h, hipStream_t s);
int enqueue_query(mi355rec* h, const float* qptr, const float* query12, int64_t exclude_global,
                  int topn_asked, uint64_t* out_keys, int64_t* out_idx, float* out_score, hipStream_t s, uint32_t notify = 0) {
    // a non-streamed query between two streamed ones: a pair is not held open across it ("pairs", below)
    if (pairs_open(h)) {
        const int rc = flush_streamed(h, s);
        if (rc) return rc;
    }
    // A shard of n rows has at most n results (the reference's heap never grows
    // past N-1, Recommender.cu:300): run only the rounds that can produce keys and
    // pad the rest, so an absurd topn costs a memset, not topn/1024 catalogue scans.
    const int topn = static_cast<int64_t>(topn_asked) < h->n ? topn_asked : static_cast<int>(h->n);
    if (topn < topn_asked) {
        const size_t pad = static_cast<size_t>(topn_asked - topn);
        HIP_TRY(h, hipMemsetAsync(out_keys + topn, 0, pad * sizeof(uint64_t), s));
        if (out_idx) HIP_TRY(h, hipMemsetAsync(out_idx + topn, 0xff, pad * sizeof(int64_t), s));
        if (out_score) HIP_TRY(h, hipMemsetAsync(out_score + topn, 0, pad * sizeof(float), s));
    }
    for (int done = 0; done < topn; done += kMaxTopK) {
        const int k = topn - done < kMaxTopK ? topn - done : kMaxTopK;
        const uint64_t* upper = done ? out_keys + done - 1 : nullptr;
        int lists = 0;
        // a notifying query (single round, its caller polls the completion word): scan, merge and the word in ONE launch
        LoneTail lone{h->d_lone_ctr, out_keys, out_idx, out_score, h->hd_done, notify, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};   // (bases: enqueue_scan)
        bool fused = false;
        int rc = enqueue_scan(h, qptr, query12, exclude_global, k, upper, s, &lists, (notify && h->d_lone_ctr) ? &lone : nullptr, &fused);
        if (rc) return rc;
        if (fused) {
            ++h->lone_fused;
            continue;
        }
        // (a notifying merge is only asked for single-round queries: it is the last launch of the call)
        rc = enqueue_merge(h, h->d_block_lists, lists, k, k, out_keys + done,
                           out_idx ? out_idx + done : nullptr, out_score ? out_score + done : nullptr, s, notify);
        if (rc) return rc;
    }
    return MI355REC_OK;
}

// Waits for the completion word of a notifying merge (a relaxed spin on pinned host memory); the stream
// is asked now and then so that a failed launch cannot hang the caller.
int wait_done(mi355rec* h, uint32_t want) {
    for (uint64_t spins = 1;; ++spins) {
        if (__atomic_load_n(h->h_done, __ATOMIC_ACQUIRE) == want) return MI355REC_OK;
        __builtin_ia32_pause();
        if ((spins & 0x3ffff) == 0) {   // every ~1 ms
            const hipError_t e = hipStreamQuery(h->stream);
            if (e == hipSuccess) {
                if (__atomic_load_n(h->h_done, __ATOMIC_ACQUIRE) == want) return MI355REC_OK;
                return fail(h, MI355REC_ERR_HIP, "the query's stream drained without its completion word");
            }
            if (e != hipErrorNotReady) return fail(h, MI355REC_ERR_HIP, "hipStreamQuery: %s", hipGetErrorString(e));
        }
    }
}

// ---- streamed single queries -------------------------------------------------------
// A stream of single queries runs ONE CALL BEHIND: query k is launched by call k + 1 (or by the flush), and its launch
// carries, beside the scanners, the merger of query k - 1's lists (one workgroup) and — where the launch can spare
// them — the seed riders and the neighbourhood workgroup of query k + 1 (handoff.hip.h), so that every launch starts
// from a launch-wide bound without a sample launch of its own.  That holds for all three kinds of rows a scan can
// stream (fp32, 8-bit replica; fp16 replica in experiment builds).  One scanning workgroup fewer than the plain scan
// uses per non-scanning one, so the launch still fits the chip in one wave of workgroups.
int ensure_streamed_alloc(mi355rec* h);
int ensure_streamed(mi355rec* h) {
    if (h->streamed_ready) return MI355REC_OK;
    const int rc = ensure_streamed_alloc(h);
    if (rc != MI355REC_OK) {   // all or nothing: no half-allocated state survives a failure
        for (int i = 0; i < 2; ++i) {
            if (h->d_stream_lists[i]) (void)hipFree(h->d_stream_lists[i]);
            h->d_stream_lists[i] = nullptr;
        }
        return rc;
    }
    h->streamed_ready = true;
    return MI355REC_OK;
}

int ensure_streamed_alloc(mi355rec* h) {
    const size_t words = static_cast<size_t>(most(h, &ScanGeom::sgrid)) * kMaxTopK;
    for (int i = 0; i < 2; ++i) HIP_TRY(h, hipMalloc(&h->d_stream_lists[i], sizeof(uint64_t) * words));
    return MI355REC_OK;
}

// The merge of the streamed query whose lists wait for it, in a launch of its own.
int merge_pending(mi355rec* h, hipStream_t s) {
    h->pending = false;
    return enqueue_merge(h, h->d_stream_lists[h->pending_buf], h->pending_lists, h->pending_topn, h->pending_topn,
                         h->pending_out, nullptr, nullptr, s);
}

int launch_stashed(mi355rec* h, hipStream_t s, bool with_next, const float* next_ptr, const float* next_q,
                   int64_t next_exclude, int next_topn, int next_buf, uint32_t next_epoch_tag);

int drain_pairs(mi355rec* h, hipStream_t s);   // ("pairs", below)

// Everything the stream of single queries still holds is launched and merged: the pairs first (their queries came first), then
// the one-query path's stashed query and pending merge.  Every call that closes a stream goes through here.
int flush_single_stream(mi355rec* h, hipStream_t s);
int flush_streamed(mi355rec* h, hipStream_t s) {
    const int rc = drain_pairs(h, s);
    return rc ? rc : flush_single_stream(h, s);
}

int flush_single_stream(mi355rec* h, hipStream_t s) {
    if (h->stashed.has) {
        const int rc = launch_stashed(h, s, false, nullptr, nullptr, -1, 0, 0, 0u);
        if (rc) return rc;
    }
    return h->pending ? merge_pending(h, s) : MI355REC_OK;
}

// Launches the stashed streamed query: scanners + the riding merger of the query before it + (with_next) the seed
// riders and the neighbourhood workgroup of the query after it, where the launch over its kind of rows has them
// (ScanGeom: riders, nbhd; hoists: their last one leaves that query's bound in d_stream_ctl).
int launch_stashed(mi355rec* h, hipStream_t s, bool with_next, const float* next_ptr, const float* next_q,
                   int64_t next_exclude, int next_topn, int next_buf, uint32_t next_epoch_tag) {
    auto& st = h->stashed;
    const bool next_bucketed = with_next && use_bucket(h, st.kind, next_topn, h->geom_bucket.riders > 0);
    const ScanGeom& g = stream_geom(h, st.kind, next_bucketed);
    // The fp32 scan's riding merger keeps 2048 survivors; with ~770 lists and topN near 1000 about
    // 2.2 topN keys survive its first cut, and an overflow drops into the exact radix select over all
    // keys in global memory (correct, ~1 ms).  Such a query's merge gets its own launch instead.
    if (st.kind == kFp32 && h->pending && h->pending_topn > kRideTopnMax) {
        const int rc = merge_pending(h, s);
        if (rc) return rc;
    }
    ScanLaunch L;
    L.kind = st.kind;
    L.streamed = true;
    const int buf = h->pending ? 1 - h->pending_buf : 0;
    if (h->pending) L.prev = PrevMerge{h->d_stream_lists[h->pending_buf], h->pending_lists, h->pending_topn, h->pending_out};
    int scanners = g.sgrid;
    L.iters = g.siters;
    if (with_next && (g.riders > 0 || g.nbhd)) {
        scanners = g.r_scan;
        L.iters = g.r_iters;
        L.next = make_next_seed(h, st.kind, g.riders, g.nbhd, next_ptr, next_q, next_exclude, next_topn, next_epoch_tag,
                                h->d_stream_seed[next_buf], g.hoists ? h->d_stream_ctl + next_buf : nullptr, h->ctl_done[next_buf],
                                next_bucketed);
    }
    L.grid = scanners + 1 + L.next.n_wgs + L.next.nbhd;
    L.lists = h->d_stream_lists[buf];
    L.sample = h->d_stream_seed[st.seed_buf];
    L.bound = st.cutoff_ready ? &h->d_stream_ctl[st.seed_buf].cutoff : nullptr;
    L.epoch = st.epoch;
    L.bucketed = st.bucketed;
    const int rc = launch_scan(h, L, st.qptr, st.q, st.exclude, st.topn, s);
    if (rc) return rc;
    // (the books move only once the launch is known to have been accepted; the riders' arrival counter counts up
    // and is never reset)
    if (L.next.ctl) h->ctl_done[next_buf] += static_cast<unsigned>(L.next.n_wgs);
    h->pending = true;
    h->pending_buf = buf;
    h->pending_topn = st.topn;
    h->pending_out = st.out;
    h->pending_lists = scanners;
    st.has = false;
    return MI355REC_OK;
}

// The one-query path: what a streamed query takes that finds no partner ("pairs", below), or whose handle does not pair.
// accepted_kind >= 0: the rows the query was accepted for when it was called (a first query of a pair that lost its partner:
// it streams what it would have streamed had it been stashed here at once).
int enqueue_streamed_single(mi355rec* h, const float* qptr, const float* query12, int64_t exclude_global, int topn,
                            uint64_t* out_keys, hipStream_t s, int accepted_kind = -1) {
    int rc = MI355REC_OK;
    if (MI355REC_EXP_FLAG("MI355REC_EXP_RIDE_NOMERGE") && h->pending) {
        rc = flush_single_stream(h, s);
        if (rc) return rc;
    }
    // One call behind: the query of the PREVIOUS call is launched now, and its launch takes the sample and the
    // neighbourhood of this one.  The first query of a stream needs a sample launch of its own.
    const int kind = accepted_kind >= 0 ? accepted_kind : single_kind(h, nullptr);
    int seed_buf = 0;
    bool sampled = false, nbhd_taken = false;
    const uint32_t epoch = next_epoch(h);   // the tag of this query's sample values and bound
    // (carried: the launch of the stashed query has riders for this one — what launch_stashed decides by as well)
    const bool bucketed = use_bucket(h, kind, topn, h->stashed.has && h->stashed.kind == kind && h->geom_bucket.riders > 0);
    const ScanGeom& ng = stream_geom(h, kind, bucketed);   // of the launch that carries THIS query's sample
    if (kind == kQ8) h->last_sample = bucketed ? MI355REC_SAMPLE_BUCKETED : MI355REC_SAMPLE_STRIDED;
    if (h->stashed.has) {
        seed_buf = 1 - h->stashed.seed_buf;
        // the riders of a launch sample the rows that launch scans: a change of rows (mi355rec_set_replica) between two
        // calls costs the next query a sample launch of its own
        const bool same = h->stashed.kind == kind;
        sampled = same && ng.riders > 0;
        nbhd_taken = same && ng.nbhd;
        rc = launch_stashed(h, s, same, qptr, query12, exclude_global, topn, seed_buf, epoch);
        if (rc) return rc;
    }
    bool bound_ready = sampled && ng.hoists;
    if (!sampled) {   // first query of a stream, or a shard too small to spare riders
        if (kind == kFp32) {
            if (h->n >= kF32LoneSeedMinRows)
                bound_ready = enqueue_f32_seed(h, qptr, query12, exclude_global, topn, h->d_stream_seed[seed_buf], h->d_stream_ctl + seed_buf,
                                               &h->ctl_done[seed_buf], epoch, s);
        } else if (!nbhd_taken) {
            enqueue_half_seed(h, kind, qptr, query12, exclude_global, topn, h->d_stream_seed[seed_buf], epoch, s, bucketed);
        }
        HIP_TRY(h, hipGetLastError());
    }
    auto& st = h->stashed;
    st.has = true;
    st.qptr = qptr;
    if (!qptr) std::memcpy(st.q, query12, sizeof st.q);
    st.exclude = exclude_global;
    st.topn = topn;
    st.out = out_keys;
    st.seed_buf = seed_buf;
    st.epoch = epoch;
    st.kind = kind;
    st.bucketed = bucketed;
    st.cutoff_ready = bound_ready;
    return MI355REC_OK;
}

// ---- pairs ----------------------------------------------------------------------------------------------------------
// Two queued single queries each stream the same 8-bit replica; the vector work per query is small beside the stream.  So
// two CONSECUTIVE streamed queries that both take the 8-bit replica and ask for the same topn <= kPairMaxTopk form a PAIR,
// and one launch (scan_q8_kernel_pair) scores every tile against both.  Either may be by row, by value or by pointer.
//
// The stream then runs up to THREE calls behind: it holds the pair that waits for its launch and the first query of the
// pair after it.  Call 2k + 1 completes pair k and launches pair k - 1, whose launch carries the two mergers of pair k - 2
// and the seed riders and neighbourhood workgroups of BOTH queries of pair k (each with its own sample buffer, SeedCtl and
// epoch; bucketed where use_bucket says so).  The first pair of a stream gets sample launches of its own.  A query that
// finds no partner — the odd tail at a flush, a change of topn, of the rows single queries stream, of mi355rec_set_replica
// or mi355rec_set_sample between the two calls, a handle that does not pair — goes through the one-query path above,
// unchanged.  The two paths are never open at once: whichever a query takes closes the other first, so keys are always
// written in call order.  All per-QUERY books stay per query; a pair launch counts once in stream_pair_launches (a launch
// that serves two pairs twice, and once in stream_group_launches).
//
// GROUPS.  Where the handle forms groups (MI355REC_PAIRING_GROUPS; AUTO from MI355REC_GROUPS_AUTO_MIN_ROWS rows), every stage
// below holds up to TWO pairs and one launch serves both (scan_q8_kernel_pair, pairs == 2: twin workgroups, one per pair, read
// every tile at nearly the same time on one XCD).  The group that forms closes at four queries — or at two where a query by
// POINTER is among them or among the queries that wait for their launch (its memory is read at most three calls after its
// call, as under pairs), and at whatever complete pairs it holds when the stream drains.  The stream then runs up to SEVEN
// calls behind.  A group of one pair is the pair launch, bit for bit and launch for launch.
bool pairing_on(const mi355rec* h) {
    if (h->pairing == MI355REC_PAIRING_ON || h->pairing == MI355REC_PAIRING_GROUPS) return true;
    if (h->pairing == MI355REC_PAIRING_OFF) return false;
    return h->n >= MI355REC_PAIRING_AUTO_MIN_ROWS;
}
bool groups_on(const mi355rec* h) {
    if (h->pairing == MI355REC_PAIRING_GROUPS) return true;
    return h->pairing == MI355REC_PAIRING_AUTO && h->n >= MI355REC_GROUPS_AUTO_MIN_ROWS;
}
bool pairs_open(const mi355rec* h) { return h->pairs.n_wait > 0 || h->pairs.n_form > 0 || h->pairs.n_pending > 0; }

void free_pairs(mi355rec* h) {
    auto& P = h->pairs;
    for (int i = 0; i < 8; ++i) {
        if (P.lists[i]) (void)hipFree(P.lists[i]);
        if (P.seed[i]) (void)hipFree(P.seed[i]);
        P.lists[i] = nullptr;
        P.seed[i] = nullptr;
    }
    if (P.ctl) (void)hipFree(P.ctl);
    P.ctl = nullptr;
    P.ready = false;
}

int ensure_pairs_alloc(mi355rec* h) {
    auto& P = h->pairs;
    const size_t words = static_cast<size_t>(h->geom[kQ8].grid > 0 ? h->geom[kQ8].grid : 1) * kPairMaxTopk;
    for (int i = 0; i < 8; ++i) {
        HIP_TRY(h, hipMalloc(&P.lists[i], sizeof(uint64_t) * words));
        HIP_TRY(h, hipMalloc(&P.seed[i], sizeof(unsigned long long) * kSampleSlots));
        HIP_TRY(h, hipMemset(P.seed[i], 0, sizeof(unsigned long long) * kSampleSlots));
    }
    HIP_TRY(h, hipMalloc(&P.ctl, sizeof(SeedCtl) * 8));
    HIP_TRY(h, hipMemset(P.ctl, 0, sizeof(SeedCtl) * 8));
    return MI355REC_OK;
}
int ensure_pairs(mi355rec* h) {
    if (h->pairs.ready) return MI355REC_OK;
    const int rc = ensure_pairs_alloc(h);
    if (rc != MI355REC_OK) {   // all or nothing
        free_pairs(h);
        return rc;
    }
    for (unsigned& d : h->pairs.ctl_done) d = 0u;
    h->pairs.ready = true;
    return MI355REC_OK;
}

// The mergers of the pairs launched last, in launches of their own and in call order.
int merge_pair_pending(mi355rec* h, hipStream_t s) {
    auto& P = h->pairs;
    const int count = P.n_pending;
    P.n_pending = 0;
    for (int x = 0; x < count; ++x) {
        const int rc = enqueue_merge(h, P.lists[4 * P.pending_set + x], P.pending_lists, P.pending_topn, P.pending_topn, P.pending_out[x],
                                     nullptr, nullptr, s);
        if (rc) return rc;
    }
    return MI355REC_OK;
}

// Launches the waiting pair, or the waiting group's two pairs: scanners + the riding mergers of the pairs before + (n_next > 0)
// the seed riders and the neighbourhood workgroups of the n_next queries after, where the launch has them (ScanGeom: riders,
// nbhd, hoists).  The launch has two slots for mergers and for queries after — four where it scans for two pairs, merges two or
// carries two; a slot nobody fills costs its few workgroups an early return.
int launch_pairs(mi355rec* h, hipStream_t s, const mi355rec::Stashed* next, int n_next, bool next_bucketed) {
    auto& P = h->pairs;
    const int n_scan = P.n_wait;   // queries this launch scans for: 2 or 4
    const int pairs = n_scan / 2;
    const int topn = P.wait[0].topn;
    // mergers in one launch write their keys in no particular order: lists that share an output are merged one after the other
    if (P.n_pending) {
        bool shared = false;
        for (int x = 0; x < P.n_pending; ++x)
            for (int y = x + 1; y < P.n_pending; ++y) {
                const uint64_t* lo = P.pending_out[x] < P.pending_out[y] ? P.pending_out[x] : P.pending_out[y];
                const uint64_t* hi = P.pending_out[x] < P.pending_out[y] ? P.pending_out[y] : P.pending_out[x];
                shared = shared || hi < lo + P.pending_topn;
            }
        if (shared) {
            const int rc = merge_pair_pending(h, s);
            if (rc) return rc;
        }
    }
    const int side_queries = (pairs == 2 || P.n_pending == 4 || n_next == 4) ? 4 : 2;
    const ScanGeom& g = stream_geom(h, kQ8, n_next > 0 && next_bucketed);
    const bool riders = n_next > 0 && (g.riders > 0 || g.nbhd);
    const int extra = side_queries * (1 + (riders ? g.riders + (g.nbhd ? 1 : 0) : 0));
    const int64_t tiles = (h->n + Q8PairConfig::kTileRows - 1) / Q8PairConfig::kTileRows;
    // every pair gets `slots` scanning workgroups and as many lists per query; twins (one per pair) share a slot's tiles, so two
    // pairs split what the chip holds at once, not what one pair would launch (a small shard's grid is its tile count)
    int64_t slots = pairs == 2 ? (g.cap - extra) / 2 : g.grid - extra;
    if (slots > kRideMaxLists - 1) slots = kRideMaxLists - 1;
    if (slots > tiles) slots = tiles;
    if (pairs == 2 && slots >= 8) slots &= ~static_cast<int64_t>(7);   // (scan_q8_kernel_pair: twins lie 8 block ids apart)
    if (slots < 1) slots = 1;
    const int64_t scanners = slots * pairs;
    const int iters = static_cast<int>((tiles + slots - 1) / slots);
    const int set = P.n_pending ? 1 - P.pending_set : 0;
    Q8PairSide side;
    std::memset(&side, 0, sizeof side);
    side.queries = side_queries;
    for (int x = 0; x < 4; ++x) side.prev[x] = no_prev_merge();
    for (int x = 0; x < P.n_pending; ++x)
        side.prev[x] = PrevMerge{P.lists[4 * P.pending_set + x], P.pending_lists, P.pending_topn, P.pending_out[x]};
    if (riders) {
        for (int x = 0; x < n_next; ++x)
            side.next[x] = make_next_seed(h, kQ8, g.riders, g.nbhd, next[x].qptr, next[x].q, next[x].exclude, next[x].topn, next[x].epoch,
                                          P.seed[next[x].seed_buf], g.hoists ? P.ctl + next[x].seed_buf : nullptr,
                                          P.ctl_done[next[x].seed_buf], next_bucketed);
        // (the kernel reads the riders' geometry from slot 0, and an unfilled slot by its null `out`)
        for (int x = n_next; x < side_queries; ++x) {
            side.next[x].n_wgs = side.next[0].n_wgs;
            side.next[x].nbhd = side.next[0].nbhd;
        }
    }
    Q8PairArgs args;
    std::memset(&args, 0, sizeof args);
    for (int x = 0; x < n_scan; ++x) {
        const mi355rec::Stashed& q = P.wait[x];
        Q8PairArg& a = args.q[x];
        a.qarg = make_query_arg(h, q.qptr, q.q);
        a.query_ptr = q.qptr;
        a.exclude_global = q.exclude;
        a.block_lists = P.lists[4 * set + x];
        a.seed_vals = P.seed[q.seed_buf];
        a.cutoff_ready = q.cutoff_ready ? &P.ctl[q.seed_buf].cutoff : nullptr;
        a.n_seed = q8_seed_count(h, q.bucketed);   // (negative: exact values)
        a.epoch = q.epoch;
    }
    const dim3 grid(static_cast<unsigned>(scanners + side_queries * (1 + side.next[0].n_wgs + side.next[0].nbhd)));
    LAUNCH_TIMED(h, h->ev_scan, h->n_scan_pairs, h->scan_launches, scan_q8_kernel_pair<Q8PairConfig>, grid, dim3(Q8PairConfig::kBlock), s,
                 h->d_feats, h->d_q8, h->n, iters, h->row_base, args, pairs, topn, h->d_half_rescored, side);
    HIP_TRY(h, hipGetLastError());
    // (the books move only once the launch is known to have been accepted: per QUERY, as on the one-query path)
    h->half_scans += n_scan;
    h->q8_scans += n_scan;
    h->routes.q8 += n_scan;
    h->stream_pair_launches += pairs;
    if (pairs == 2) ++h->stream_group_launches;
    for (int x = 0; x < n_next; ++x)
        if (side.next[x].ctl) P.ctl_done[next[x].seed_buf] += static_cast<unsigned>(side.next[x].n_wgs);
    P.n_pending = n_scan;
    P.pending_set = set;
    P.pending_lists = static_cast<int>(slots);
    P.pending_topn = topn;
    for (int x = 0; x < n_scan; ++x) P.pending_out[x] = P.wait[x].out;
    P.n_wait = 0;
    return MI355REC_OK;
}

// The first `count` (2 or 4) queries of the group that forms become the waiting stage: the pairs that waited are launched now,
// and their launch takes the samples and the neighbourhoods of these.  The first pairs of a stream, and a shard too small to
// spare riders, get sample launches of their own.  (Which sample: what use_bucket gives a CARRIED query — also for the first
// pairs of a stream.  Their sample launches are not on the critical path as a query alone's is: the launch is calls away.)
int close_forming(mi355rec* h, hipStream_t s, int count) {
    auto& P = h->pairs;
    const int topn = P.form[0].topn;
    const int set = P.n_wait ? 1 - (P.wait[0].seed_buf >> 2) : 0;
    const bool bucketed = use_bucket(h, kQ8, topn, h->geom_bucket.riders > 0);
    const ScanGeom& ng = stream_geom(h, kQ8, bucketed);   // of the launch that carries THESE queries' samples
    mi355rec::Stashed nx[4];
    for (int i = 0; i < count; ++i) {
        nx[i] = P.form[i];
        nx[i].seed_buf = 4 * set + i;
        nx[i].epoch = next_epoch(h);
        nx[i].bucketed = bucketed;
    }
    h->last_sample = bucketed ? MI355REC_SAMPLE_BUCKETED : MI355REC_SAMPLE_STRIDED;
    bool sampled = false;
    if (P.n_wait) {
        sampled = ng.riders > 0;
        const int rc = launch_pairs(h, s, nx, count, bucketed);
        if (rc) return rc;
    }
    if (!sampled) {
        for (int i = 0; i < count; ++i)
            enqueue_half_seed(h, kQ8, nx[i].qptr, nx[i].q, nx[i].exclude, topn, P.seed[nx[i].seed_buf], nx[i].epoch, s, bucketed);
        HIP_TRY(h, hipGetLastError());
    }
    for (int i = 0; i < count; ++i) {
        nx[i].cutoff_ready = sampled && ng.hoists;
        P.wait[i] = nx[i];
    }
    P.n_wait = count;
    for (int i = count; i < P.n_form; ++i) P.form[i - count] = P.form[i];
    P.n_form -= count;
    return MI355REC_OK;
}

// Everything the pairs still hold, in call order: the complete pair among the queries of the group that forms (it closes
// here), the waiting pairs, the mergers, and the one query left without a partner — which takes the one-query path (left
// open: the caller flushes it or streams on).
int drain_pairs(mi355rec* h, hipStream_t s) {
    auto& P = h->pairs;
    if (P.n_form >= 2) {
        const int rc = close_forming(h, s, 2);
        if (rc) return rc;
    }
    if (P.n_wait) {
        const int rc = launch_pairs(h, s, nullptr, 0, false);
        if (rc) return rc;
    }
    if (P.n_pending) {
        const int rc = merge_pair_pending(h, s);
        if (rc) return rc;
    }
    if (P.n_form) {
        const mi355rec::Stashed f = P.form[0];
        P.n_form = 0;
        return enqueue_streamed_single(h, f.qptr, f.q, f.exclude, f.topn, f.out, s, h->d_q8 ? f.kind : -1);
    }
    return MI355REC_OK;
}

int enqueue_streamed(mi355rec* h, const float* qptr, const float* query12, int64_t exclude_global, int topn,
                     uint64_t* out_keys, hipStream_t s) {
    int rc = ensure_streamed(h);
    if (rc) return rc;
    rc = flush_mstream(h, s);   // a stream of BATCHES on this handle is closed first
    if (rc) return rc;
    auto& P = h->pairs;
    bool pair = single_kind(h, nullptr) == kQ8 && topn <= kPairMaxTopk && pairing_on(h);
    if (pair && ensure_pairs(h) != MI355REC_OK) {   // (no room for the pairs' buffers: the one-query path serves)
        (void)hipGetLastError();
        pair = false;
    }
    // queries whose partner this one cannot be find none
    if (pair && P.n_form && (P.form[0].topn != topn || P.first_replica_mode != h->replica_mode || P.first_sample_mode != h->sample_mode)) {
        rc = drain_pairs(h, s);
        if (rc) return rc;
    }
    if (!pair) {
        if (pairs_open(h)) {
            rc = drain_pairs(h, s);
            if (rc) return rc;
        }
        return enqueue_streamed_single(h, qptr, query12, exclude_global, topn, out_keys, s);
    }
    if (h->stashed.has || h->pending) {
        rc = flush_single_stream(h, s);
        if (rc) return rc;
    }
    mi355rec::Stashed x;
    x.has = true;
    x.qptr = qptr;
    if (!qptr) std::memcpy(x.q, query12, sizeof x.q);
    x.exclude = exclude_global;
    x.topn = topn;
    x.out = out_keys;
    x.kind = kQ8;
    // (a pointer into the handle's own rows is a query by row; any other is the caller's memory, read when the launch runs)
    x.by_pointer = qptr && !(qptr >= h->d_feats && qptr < h->d_feats + h->n * kDim);
    if (P.n_form >= 2 && !groups_on(h)) {   // (the handle stopped forming groups while a pair waited for a second one)
        rc = close_forming(h, s, 2);
        if (rc) return rc;
    }
    if (!P.n_form) {
        P.first_replica_mode = h->replica_mode;
        P.first_sample_mode = h->sample_mode;
    }
    P.form[P.n_form++] = x;   // it waits for its partners without a sample
    if (P.n_form & 1) return MI355REC_OK;
    // (which sample a complete pair will take is known now, whenever its group closes — close_forming asks the same question,
    // and a change of mi355rec_set_sample in between drains these queries — so mi355rec_bucket_sample_info answers at the call
    // that completes a pair, as it does where the handle forms no groups)
    h->last_sample = use_bucket(h, kQ8, topn, h->geom_bucket.riders > 0) ? MI355REC_SAMPLE_BUCKETED : MI355REC_SAMPLE_STRIDED;
    // A complete pair.  Does the group close here?  At two pairs — or at one where the handle forms no groups, and where a query
    // by pointer is in the group or waits for its launch: that launch is then two calls away at the most, as under pairs.
    bool closes = P.n_form == 4 || !groups_on(h);
    // AUTO: the head of a stream runs as pairs — the first pair takes its samples at once and the second one launches it, as
    // where the handle forms no groups — and groups form once a launch of the stream is under way.  (A short stream gained
    // nothing from groups otherwise: four sample launches and eight calls before its first scan.  GROUPS groups from the start.)
    if (h->pairing == MI355REC_PAIRING_AUTO && P.n_pending == 0) closes = true;
    for (int i = 0; i < P.n_form; ++i) closes = closes || P.form[i].by_pointer;
    for (int i = 0; i < P.n_wait; ++i) closes = closes || P.wait[i].by_pointer;
    return closes ? close_forming(h, s, P.n_form) : MI355REC_OK;
}

}  // namespace
