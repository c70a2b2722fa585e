// engine_sync.hip.h — the ONE result path of the synchronous host API.  Every synchronous call (a single query, a batch, a
// filtered query, a playlist request, a re-rank) makes sure the handle's result slots are large enough, joins the handle's
// own stream, decides where its last launch stores the ids and scores (small results: straight into pinned host memory) and
// whether that launch raises the completion word the host spins on; after its launches it waits, copies the results into
// the caller's buffers and pads them.  sync_begin is the first half, sync_finish the second; the launches in between are
// the caller's.  (Part of mi355rec.hip's translation unit, included after engine_single.hip.h.)
#pragma once

#include "engine_single.hip.h"
#include "playlist_request.h"

namespace {

// The value the next notifying launch stores in the completion word (never 0: the word starts as 0).
uint32_t next_done_seq(mi355rec* h) {
    if (++h->done_seq == 0u) ++h->done_seq;
    return h->done_seq;
}

// What one synchronous call knows about its result slots between sync_begin and sync_finish.
struct SyncSlots {
    int eff = 0;            // results per query: what the rows can return at most, not what the caller's buffers hold
    int batch = 1;
    bool direct = false;    // batch * eff <= kDirectResultSlots: the launches store into pinned host memory, no D2H copies
    uint32_t want = 0;      // != 0: the call's last launch raises the completion word to this value and the host spins on it
    int64_t* idx = nullptr;   // where the launches store: h->hd_idx / hd_score when direct, h->d_idx / d_score otherwise
    float* score = nullptr;
};

// The slots for `batch` lists of `eff` results, and the handle's own stream behind whatever the caller enqueued through the
// handle.  The call notifies (want != 0) under ONE rule: may_notify && direct && 0 < eff <= kMaxTopK && batch == 1, a
// single-round call whose last launch can raise the word; a caller whose launches never do passes may_notify = false.
int sync_begin(mi355rec* h, int eff, int batch, bool may_notify, SyncSlots* ss) {
    const size_t slots = static_cast<size_t>(batch) * eff;
    int rc = ensure_slots(h, slots);
    if (!rc) rc = sync_api_begin(h);
    if (rc) return rc;
    ss->eff = eff;
    ss->batch = batch;
    ss->direct = slots <= static_cast<size_t>(kDirectResultSlots);
    ss->want = may_notify && ss->direct && eff > 0 && eff <= kMaxTopK && batch == 1 ? next_done_seq(h) : 0u;
    ss->idx = ss->direct ? h->hd_idx : h->d_idx;
    ss->score = ss->direct ? h->hd_score : h->d_score;
    return MI355REC_OK;
}

// After the call's launches: the copies back where the results are not in pinned memory yet, the wait (the completion word,
// or the stream), then per query the count of valid ids and its `eff` results into the caller's `topn`-strided buffers,
// padded with -1 / 0.0f.  out_score and out_count may be null.
int sync_finish(mi355rec* h, const SyncSlots& ss, int topn, int64_t* out_idx, float* out_score, int* out_count) {
    const size_t eff = static_cast<size_t>(ss.eff);
    if (!ss.direct) {
        HIP_TRY(h, hipMemcpyAsync(h->h_idx, h->d_idx, ss.batch * eff * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->h_score, h->d_score, ss.batch * eff * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    if (ss.want) {
        const int rc = wait_done(h, ss.want);
        if (rc) return rc;
    } else {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    for (int b = 0; b < ss.batch; ++b) {
        const int64_t* src = h->h_idx + b * eff;
        const mi355playlist::Outputs out{out_idx + static_cast<size_t>(b) * topn, out_score ? out_score + static_cast<size_t>(b) * topn : nullptr,
                                         nullptr, out_count ? out_count + b : nullptr, nullptr};
        int c = 0;
        while (c < ss.eff && src[c] >= 0) ++c;
        if (eff) {   // (an empty shard has no slots at all)
            std::memcpy(out.idx, src, eff * sizeof(int64_t));
            if (out.score) std::memcpy(out.score, h->h_score + b * eff, eff * sizeof(float));
        }
        mi355playlist::pad(out, ss.eff, topn, c);
    }
    return MI355REC_OK;
}

// The same second half for a call whose result is not a top-N list but `bytes` of a device buffer of its own ("CANDIDATE SCORES": the
// entries' keys): copied into the caller's pinned `host` on the handle's stream behind the call's launches, then the stream is
// waited for (such a call never notifies: sync_begin was given eff == 0).
int sync_finish_buffer(mi355rec* h, void* host, const void* dev, size_t bytes) {
    HIP_TRY(h, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MI355REC_OK;
}

}  // namespace
