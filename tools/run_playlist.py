"""Playlist queries at 10 M x 12, top-100, one handle, synchronous calls: p50 / p99 of mi355rec_query_playlist_topn for
K = 1, 10 and 32 members beside mi355rec_query_topn by value (exclude -1) in the same process, the rows whose K exact
chains were computed per query (mi355rec_playlist_counters) and the kernel time of playlist_scan_kernel (HIP events:
mi355rec_set_timing).  Two catalogues: uniform random rows, and 3000 contiguous clusters with the members taken from one
cluster.  Prints one JSON document and writes it to --out.

    python tools/run_playlist.py --out profiles/r07_playlist.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_playlist -o playlist -- python tools/run_playlist.py --profile
(--profile: fewer calls, the uniform catalogue only.)"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def pct(ts, p):
    return float(np.percentile(np.asarray(ts) * 1e6, p))


def timed(fn, args, warm=20):
    for x in args[:warm]:
        fn(x)
    ts = []
    for x in args:
        t0 = time.perf_counter()
        fn(x)
        ts.append(time.perf_counter() - t0)
    return {"p50_us": round(pct(ts, 50), 1), "p99_us": round(pct(ts, 99), 1), "calls": len(ts)}


def kernel_us(eng, fn, args):
    eng.set_timing(1)
    for x in args:
        fn(x)
    ms = eng.stats().last_scan_ms
    eng.set_timing(0)
    return round(ms * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.synth import clustered_catalogue

    n, topn = a.rows, a.topn
    calls = 60 if a.profile else a.calls
    rng = np.random.default_rng(7)
    out = {"rows": n, "topn": topn, "device": torch.cuda.get_device_name(0), "catalogues": {}}
    cats = ["uniform"] if a.profile else ["uniform", "clusters_3000_contiguous"]
    for cname in cats:
        if cname == "uniform":
            data = torch.rand((n, 12), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
            pick = lambda k: rng.choice(n, size=k, replace=False)   # noqa: E731
        else:
            clusters = 3000
            data = clustered_catalogue(n, 0.03, seed=4242 + clusters, clusters=clusters, contiguous=True, ramp=False)
            per = n // clusters
            pick = lambda k: int(rng.integers(0, clusters)) * per + rng.choice(per, size=k, replace=False)   # noqa: E731
        host = data.cpu().numpy()
        res = {}
        with CosineEngine(data) as eng:
            vecs = [host[int(r)] for r in rng.integers(0, n, size=calls)]
            res["by_value"] = timed(lambda q: eng.query_topn(q, -1, topn), vecs)
            for k in ((10,) if a.profile else (1, 10, 32)):
                lists = [pick(k) for _ in range(calls)]
                key = f"playlist_k{k}"
                res[key] = timed(lambda rows: eng.query_playlist_topn(rows, topn), lists)
                before = eng.playlist_counters()
                res[key]["playlist_scan_kernel_us"] = kernel_us(eng, lambda rows: eng.query_playlist_topn(rows, topn), lists[:100])
                after = eng.playlist_counters()
                res[key]["rows_exact_per_query"] = (after["rows_exact"] - before["rows_exact"]) // 100
                res[key]["ratio_to_by_value_p50"] = round(res[key]["p50_us"] / res["by_value"]["p50_us"], 3)
        del data
        torch.cuda.empty_cache()
        out["catalogues"][cname] = res
    if not a.profile:
        u, c = out["catalogues"]["uniform"], out["catalogues"]["clusters_3000_contiguous"]
        out["bars"] = {"uniform_k10_le_1p5x": u["playlist_k10"]["ratio_to_by_value_p50"] <= 1.5,
                       "uniform_k32_le_2x": u["playlist_k32"]["ratio_to_by_value_p50"] <= 2.0,
                       "clusters_k10_le_2x": c["playlist_k10"]["ratio_to_by_value_p50"] <= 2.0}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
