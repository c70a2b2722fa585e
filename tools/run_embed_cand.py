"""EMBEDDING CANDIDATE LISTS beside the two calls that serve a candidate set without them, at 10 M rows, one handle,
top-100, cosine, w_audio = 0 (include/mi355rec_embed_cand.h).  For every (d, storage) of --dims x
--storages, in ONE run on one box, over ONE table on the device, and for every list length m of --candidates, once with
uniformly random ids and once with one contiguous run of ids:

    rank     a region is --calls back-to-back CandidateEmbeddingTable.rank enqueues (a fresh list each, preallocated
             outputs) and ONE stream synchronise
    scores   the same with CandidateEmbeddingTable.scores
    scan     the same with StreamedEmbeddingTable.query: the whole table, whatever the list
    only     --calls RestrictedEmbeddingTable.query(only=the set of the same ids) calls, each its own host round trip; the
             sets are built before the region (building one is timed apart, as set_build_us: a fresh list needs a fresh set)

--regions regions of each, alternating, so that all four see the same box.  Host timers around the regions
(time.perf_counter: a region ends in a synchronise or in a synchronous call), no device events inside them.  Nothing is
fixed in advance; the expectation is derived: a rank call reads at most m x (row bytes rounded up to 128) + 8 m bytes and
its launches are small, so at 10 000 random candidates it should cost no more than `only` (margin: the spread of the only
regions of the same run) and less than `scan` at every m up to rows / 100.  Before timing, rank is held to `only`, bit for bit.

    python tools/run_embed_cand.py --out profiles/r36_embed_cand.json"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

F32 = np.float32


def region_us(run_region, per_region):
    t0 = time.perf_counter()
    run_region()
    return (time.perf_counter() - t0) * 1e6 / per_region


def measure(a, d, storage, write):
    import torch

    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_cand import CandidateEmbeddingTable
    from spotify_recommender_amd.embed_sets import RestrictedEmbeddingTable
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    n, topn, calls = a.rows, 100, a.calls
    rng = np.random.default_rng(36 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    if storage == "fp16":
        table = table.astype(np.float16)
    users = torch.from_numpy(rng.standard_normal((calls, d), dtype=F32)).to("cuda:0")
    kw = dict(metric="cosine", embed_weight=1.0)
    out = {"points": []}
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(36)
    with CosineEngine(feats) as eng:
        dev_table = torch.from_numpy(table).to("cuda:0")
        s = torch.cuda.Stream()
        with CandidateEmbeddingTable(eng, dev_table) as ct, StreamedEmbeddingTable(eng, dev_table) as st, RestrictedEmbeddingTable(eng, table) as rt:
            info = ct.info()
            out["info"] = {k: info[k] for k in ("rows", "dim", "storage_name", "device_bytes", "tile_rows", "grid", "rank_launches", "scores_call_launches")}
            ranked = (torch.empty(topn, dtype=torch.int64, device="cuda:0"), torch.empty(topn, dtype=torch.float32, device="cuda:0"),
                      torch.empty((), dtype=torch.int32, device="cuda:0"))
            scanned = tuple(torch.empty_like(x) for x in ranked)

            def scan_region():
                for i in range(calls):
                    st.query(users[i], out=scanned, stream=s, topn=topn, **kw)
                s.synchronize()

            for m in a.candidates:
                valued = (torch.empty(m, dtype=torch.float32, device="cuda:0"), torch.empty(m, dtype=torch.float32, device="cuda:0"),
                          torch.empty(m, dtype=torch.uint8, device="cuda:0"))
                for pattern in ("random", "contiguous"):
                    if pattern == "random":
                        lists = torch.randint(0, n, (calls, m), dtype=torch.int64, device="cuda:0", generator=gen)
                    else:
                        starts = torch.randint(0, n - m + 1, (calls, 1), dtype=torch.int64, device="cuda:0", generator=gen)
                        lists = starts + torch.arange(m, dtype=torch.int64, device="cuda:0")[None, :]
                    host_lists = lists.cpu().numpy()
                    host_users = users.cpu().numpy()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sets = [rt.rowset(host_lists[i]) for i in range(calls)]
                    set_build_us = (time.perf_counter() - t0) * 1e6 / calls

                    def rank_region():
                        for i in range(calls):
                            ct.rank(users[i], lists[i], out=ranked, stream=s, topn=topn, **kw)
                        s.synchronize()

                    def scores_region():
                        for i in range(calls):
                            ct.scores(users[i], lists[i], out=valued, stream=s, **kw)
                        s.synchronize()

                    def only_region():
                        for i in range(calls):
                            rt.query(user=host_users[i], only=sets[i], topn=topn, **kw)

                    # the same answers first (the last call of a region is what `ranked` holds); every region once, warm
                    rank_region()
                    wi, ws = rt.query(user=host_users[-1], only=sets[-1], topn=topn, **kw)
                    assert int(ranked[2]) == wi.size and ranked[0][: wi.size].cpu().tolist() == wi.tolist()
                    assert np.array_equal(ranked[1][: wi.size].cpu().numpy().view(np.uint32), ws.view(np.uint32))
                    scores_region(), scan_region(), only_region()
                    t = {"scan": [], "only": [], "rank": [], "scores": []}
                    for _ in range(a.regions):   # alternating, so that all see the same box
                        t["scan"].append(region_us(scan_region, calls))
                        t["only"].append(region_us(only_region, calls))
                        t["rank"].append(region_us(rank_region, calls))
                        t["scores"].append(region_us(scores_region, calls))
                    for x in sets:
                        x.close()
                    med = {k: float(np.median(v)) for k, v in t.items()}
                    point = {"m": m, "pattern": pattern, "set_build_us": round(set_build_us, 1),
                             "only_spread_us": round(max(t["only"]) - min(t["only"]), 1),
                             "rank_no_more_than_only": bool(med["rank"] <= med["only"] + max(t["only"]) - min(t["only"])),
                             "rank_less_than_scan": bool(med["rank"] < med["scan"])}
                    for k, v in t.items():
                        point[f"{k}_us_per_call"] = [round(x, 1) for x in v]
                        point[f"{k}_median_us"] = round(med[k], 1)
                    out["points"].append(point)
                    print(json.dumps({"d": d, "storage": storage, **{k: point[k] for k in point if not k.endswith("per_call")}}), flush=True)
                    write(out)
                    del lists, sets
    for pattern in ("random", "contiguous"):   # the first m at which the gather stops beating the ONLY-set call
        pts = [p for p in out["points"] if p["pattern"] == pattern]
        lost = [p["m"] for p in pts if p["rank_median_us"] > p["only_median_us"]]
        out[f"crossover_m_{pattern}"] = lost[0] if lost else None
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    p.add_argument("--storages", nargs="+", default=["fp32", "fp16"], choices=["fp32", "fp16"])
    p.add_argument("--candidates", type=int, nargs="+", default=[100, 1_000, 10_000, 100_000, 1 << 20])
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--regions", type=int, default=5)
    p.add_argument("--out", default="profiles/r36_embed_cand.json")
    a = p.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    result = {"rows": a.rows, "topn": 100, "metric": "cosine", "calls_per_region": a.calls, "regions": a.regions,
              "device": torch.cuda.get_device_name(0), "tables": {}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for d in a.dims:
        for storage in a.storages:
            def write(partial, key=f"d{d}_{storage}"):
                result["tables"][key] = partial
                Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
            write(measure(a, d, storage, write))


if __name__ == "__main__":
    main()
