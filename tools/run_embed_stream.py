"""STREAMED EMBEDDING REQUESTS beside the synchronous libraries at 10 M rows, one handle, top-100, cosine, w_audio = 0
(include/mi355rec_embed_stream.h).  For d in --dims, in ONE run on one box, over ONE table on the device:

    single   a region is --calls back-to-back StreamedEmbeddingTable.query enqueues (a fresh device user each, preallocated
             outputs) and ONE stream synchronise; beside it a region of --calls EmbeddingTable.query calls (each its own
             host round trip).  --regions regions of each, alternating.
    batch    the same with 64 users per call (--batch-calls calls per region) against EmbeddingBatchTable.query_users.

Host timers around the regions (time.perf_counter: a region ends in a synchronise), no device events inside them.  The
expectation is derived, not fixed: the same scan and merge, plus two launches of one workgroup per user, minus a host round
trip — so streamed time per query should not exceed synchronous time per query; the margin is the spread (max - min) of the
synchronous regions of the same run.  Before timing, the streamed answers are held to the synchronous ones, bit for bit.

    python tools/run_embed_stream.py --out profiles/r35_embed_stream.json"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

F32 = np.float32


def regions_us(run_region, regions, per_region):
    """Microseconds per call of each region."""
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        run_region()
        out.append((time.perf_counter() - t0) * 1e6 / per_region)
    return out


def summary(sync, streamed):
    spread = max(sync) - min(sync)
    med_sync, med_streamed = float(np.median(sync)), float(np.median(streamed))
    return {"sync_us_per_call": [round(x, 1) for x in sync], "streamed_us_per_call": [round(x, 1) for x in streamed],
            "sync_median_us": round(med_sync, 1), "streamed_median_us": round(med_streamed, 1), "sync_spread_us": round(spread, 1),
            "streamed_over_sync": round(med_streamed / med_sync, 3), "streamed_within_expectation": bool(med_streamed <= med_sync + spread)}


def measure(a, d):
    import torch

    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    n, topn, B = a.rows, 100, 64
    rng = np.random.default_rng(35 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    users = rng.standard_normal((a.calls, d), dtype=F32)
    batches = rng.standard_normal((a.batch_calls, B, d), dtype=F32)
    kw = dict(metric="cosine", embed_weight=1.0, topn=topn)
    out = {}
    with CosineEngine(feats) as eng:
        dev_table = torch.from_numpy(table).to("cuda:0")
        dev_users, dev_batches = torch.from_numpy(users).to("cuda:0"), torch.from_numpy(batches).to("cuda:0")
        s = torch.cuda.Stream()
        with StreamedEmbeddingTable(eng, dev_table) as st:
            info = st.info()
            out["info"] = {k: info[k] for k in ("rows", "dim", "device_bytes", "tile_rows", "grid", "pass_users", "borrowed")}
            one = (torch.empty(topn, dtype=torch.int64, device="cuda:0"), torch.empty(topn, dtype=torch.float32, device="cuda:0"),
                   torch.empty((), dtype=torch.int32, device="cuda:0"))
            many = (torch.empty((B, topn), dtype=torch.int64, device="cuda:0"), torch.empty((B, topn), dtype=torch.float32, device="cuda:0"),
                    torch.empty(B, dtype=torch.int32, device="cuda:0"))
            torch.cuda.synchronize()

            def streamed_single():
                for i in range(a.calls):
                    st.query(dev_users[i], out=one, stream=s, **kw)
                s.synchronize()

            def streamed_batch():
                for i in range(a.batch_calls):
                    st.query(dev_batches[i], out=many, stream=s, **kw)
                s.synchronize()

            with EmbeddingTable(eng, table) as base:
                # the same answers first (the last call of a region is what `one` holds)
                streamed_single()
                wi, ws = base.query(user=users[-1], **kw)
                assert one[0][: wi.size].cpu().tolist() == wi.tolist() and np.array_equal(one[1][: wi.size].cpu().numpy().view(np.uint32), ws.view(np.uint32))

                def sync_single():
                    for i in range(a.calls):
                        base.query(user=users[i], **kw)

                sync_single()   # warm
                sync, streamed = [], []
                for _ in range(a.regions):   # alternating, so that both see the same box
                    sync += regions_us(sync_single, 1, a.calls)
                    streamed += regions_us(streamed_single, 1, a.calls)
                out["single"] = summary(sync, streamed)
            with EmbeddingBatchTable(eng, table) as bbase:
                streamed_batch()
                bi, bs, _ = bbase.query_users(users=batches[-1], **kw)
                assert np.array_equal(many[0].cpu().numpy(), bi) and np.array_equal(many[1].cpu().numpy().view(np.uint32), bs.view(np.uint32))

                def sync_batch():
                    for i in range(a.batch_calls):
                        bbase.query_users(users=batches[i], **kw)

                sync_batch()
                sync, streamed = [], []
                for _ in range(a.regions):
                    sync += regions_us(sync_batch, 1, a.batch_calls)
                    streamed += regions_us(streamed_batch, 1, a.batch_calls)
                out["batch_64_users"] = summary(sync, streamed)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--batch-calls", type=int, default=200)
    p.add_argument("--regions", type=int, default=5)
    p.add_argument("--out", default="profiles/r35_embed_stream.json")
    a = p.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    result = {"rows": a.rows, "topn": 100, "metric": "cosine", "calls_per_region": a.calls, "batch_calls_per_region": a.batch_calls,
              "regions": a.regions, "device": torch.cuda.get_device_name(0), "dims": {}}
    for d in a.dims:
        result["dims"][str(d)] = measure(a, d)
        print(json.dumps({str(d): result["dims"][str(d)]}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
