"""MULTI-INTEREST EMBEDDING REQUESTS beside the K streamed single-interest calls they replace, at 10 M rows, one handle,
top-100, cosine, w_audio = 0 (include/mi355rec_embed_multi.h).  For every (d, storage) of --dims x
--storages, in ONE run on one box, over ONE table on the device, and for every K of --interests:

    multi    a region is --calls back-to-back MultiInterestEmbeddingTable.query enqueues (a fresh set of K interests each,
             preallocated outputs) and ONE stream synchronise
    single   the same with K StreamedEmbeddingTable.query enqueues per call, one per interest: K x --calls enqueues and ONE
             synchronise.  These leave K lists; the union, de-duplication and re-sort the caller would still owe is NOT in them.

--regions regions of each, alternating, so that both see the same box.  Host timers around the regions (time.perf_counter: a
region ends in a synchronise), no device events inside them.  The bar, from the project's own batch figures (a pass of 8
users costs 1.6 - 1.8 single calls): at K = 8 one multi-interest call takes less than half the time of the
8 sequential calls, at every measured width and storage.  K = 1 beside the single streamed call and the cost per added
chunk of `pass_interests` interests are recorded without a bar.  Before timing, the multi-interest answer is held to the
merge of the K single answers, bit for bit.

    python tools/run_embed_multi.py --out profiles/r37_embed_multi.json"""
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


def merged(singles, topn):
    """The merge of identity 2 over [(ids, scores)] of the K interests: union by row, the larger value, the lower k."""
    held = {}
    for k, (ids, sc) in enumerate(singles):
        for i, s in zip(ids.tolist(), sc):
            if i not in held or s > held[i][0]:
                held[i] = (s, k)
    rows = np.array(sorted(held), np.int64)
    vals = np.array([held[i][0] for i in rows.tolist()], F32)
    ks = np.array([held[i][1] for i in rows.tolist()], np.int32)
    order = np.lexsort((rows, -vals.astype(np.float64)))[:topn]
    return rows[order], vals[order], ks[order]


def measure(a, d, storage, write):
    import torch

    from spotify_recommender_amd import CosineEngine, MultiInterestEmbeddingTable
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    n, topn, calls = a.rows, 100, a.calls
    rng = np.random.default_rng(37 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    if storage == "fp16":
        table = table.astype(np.float16)
    kmax = max(a.interests)
    interests = torch.from_numpy(rng.standard_normal((calls, kmax, d), dtype=F32)).to("cuda:0")
    kw = dict(metric="cosine", embed_weight=1.0, topn=topn)
    out = {"points": []}
    with CosineEngine(feats) as eng:
        dev_table = torch.from_numpy(table).to("cuda:0")
        del table, feats
        s = torch.cuda.Stream()
        with MultiInterestEmbeddingTable(eng, dev_table) as mt, StreamedEmbeddingTable(eng, dev_table) as st:
            info = mt.info()
            out["info"] = {k: info[k] for k in ("rows", "dim", "storage_name", "device_bytes", "tile_rows", "grid", "pass_interests", "query_launches")}
            answer = (torch.empty(topn, dtype=torch.int64, device="cuda:0"), torch.empty(topn, dtype=torch.float32, device="cuda:0"),
                      torch.empty((), dtype=torch.int32, device="cuda:0"), torch.empty(topn, dtype=torch.int32, device="cuda:0"))
            scanned = tuple(torch.empty_like(x) for x in answer[:3])
            torch.cuda.synchronize()
            for K in a.interests:
                sets = [interests[i, :K].contiguous() for i in range(calls)]   # (made before the regions)
                torch.cuda.synchronize()

                def multi_region():
                    for i in range(calls):
                        mt.query(sets[i], out=answer, stream=s, **kw)
                    s.synchronize()

                def single_region():
                    for i in range(calls):
                        for k in range(K):
                            st.query(sets[i][k], out=scanned, stream=s, **kw)
                    s.synchronize()

                # the same answers first (the last call of a region is what `answer` holds); every region once, warm
                multi_region()
                singles = []
                for k in range(K):
                    i1, s1, c1 = st.query(sets[-1][k], stream=s, **kw)
                    s.synchronize()
                    singles.append((i1[: int(c1)].cpu().numpy(), s1[: int(c1)].cpu().numpy()))
                wi, ws, wk = merged(singles, topn)
                assert int(answer[2]) == wi.size and answer[0][: wi.size].cpu().tolist() == wi.tolist()
                assert np.array_equal(answer[1][: wi.size].cpu().numpy().view(np.uint32), ws.view(np.uint32))
                assert answer[3][: wi.size].cpu().tolist() == wk.tolist()
                single_region()
                t = {"multi": [], "single": []}
                for _ in range(a.regions):   # alternating, so that both see the same box
                    t["single"].append(region_us(single_region, calls))
                    t["multi"].append(region_us(multi_region, calls))
                med = {k: float(np.median(v)) for k, v in t.items()}
                point = {"K": K, "ratio": round(med["multi"] / med["single"], 3)}
                if K == 8:
                    point["less_than_half_of_8_single_calls"] = bool(med["multi"] < 0.5 * med["single"])
                for k, v in t.items():
                    point[f"{k}_us_per_call"] = [round(x, 1) for x in v]
                    point[f"{k}_median_us"] = round(med[k], 1)
                out["points"].append(point)
                print(json.dumps({"d": d, "storage": storage, **{k: point[k] for k in point if not k.endswith("per_call")}}), flush=True)
                write(out)
                del sets
    # the cost of one more chunk of pass_interests interests: the slope of the multi-interest medians between the two largest K
    pts = sorted(out["points"], key=lambda p: p["K"])
    if len(pts) >= 2:
        lo, hi = pts[-2], pts[-1]
        out["us_per_added_chunk"] = round((hi["multi_median_us"] - lo["multi_median_us"]) / (hi["K"] - lo["K"]) * out["info"]["pass_interests"], 1)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    p.add_argument("--storages", nargs="+", default=["fp32", "fp16"], choices=["fp32", "fp16"])
    p.add_argument("--interests", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--regions", type=int, default=5)
    p.add_argument("--out", default="profiles/r37_embed_multi.json")
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
