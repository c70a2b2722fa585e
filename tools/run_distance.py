"""DISTANCE REQUESTS at 10 M x 12, top-100, one handle, synchronous calls (include/mi355rec_diag.h, DISTANCE REQUESTS; DESIGN.md
5.4.10).  In one process, on one handle over uniform random rows, K = 1 by row, three calls side by side:
    cosine          the cosine playlist request of the same shape (12 B per row over the 8-bit replica);
    cosine_prior    the same request with MI355REC_PQ_PRIOR (uniform priors, beta = 0.25): 12 + 4 B per row, a per-row cut;
    distance        the distance request: 12 + 4 B per row (the norms), a per-row cut.
The three alternate region by region (a region = --calls synchronous calls, each ending in the host's wait for the result);
per case the median over the regions of the region's mean call time, the spread of the regions, the scan kernel's time (HIP
events: mi355rec_set_timing, a run of its own), and the rows whose chains were computed per query
(mi355rec_playlist_counters).  Then the same distance request on a handle without a replica (every row exact).
Prints one JSON document and writes it to --out.

    python tools/run_distance.py --out profiles/r14_distance.json"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def region(fn, args):
    t0 = time.perf_counter()
    for x in args:
        fn(x)                                  # (synchronous: returns when the results are on the host)
    return (time.perf_counter() - t0) / len(args) * 1e6


def kernel_us(eng, fn, args):
    eng.set_timing(1)
    for x in args:
        fn(x)
    ms = eng.stats().last_scan_ms
    eng.set_timing(0)
    return round(ms * 1e3, 1)


def measure(eng, cases, lists, regions, calls):
    """{name: figures}: the cases alternate region by region over the same member rows."""
    for fn in cases.values():                  # warm-up: every shape the timed regions use (and the norms' build)
        for x in lists[:20]:
            fn(x)
    times = {name: [] for name in cases}
    for r in range(regions):
        chunk = lists[r * calls:(r + 1) * calls]
        for name, fn in cases.items():
            times[name].append(region(fn, chunk))
    out = {}
    for name, fn in cases.items():
        ts = np.asarray(times[name])
        before = eng.playlist_counters()
        k_us = kernel_us(eng, fn, lists[:50])
        after = eng.playlist_counters()
        out[name] = {"call_us_median_of_regions": round(float(np.median(ts)), 1), "call_us_min": round(float(ts.min()), 1),
                     "call_us_max": round(float(ts.max()), 1), "regions": regions, "calls_per_region": calls,
                     "playlist_scan_kernel_us": k_us, "rows_exact_per_query": (after["rows_exact"] - before["rows_exact"]) // 50}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed region")
    ap.add_argument("--regions", type=int, default=7, help="timed regions per case (at least 5)")
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions: at least 5")
    import torch
    from spotify_recommender_amd import CosineEngine, build, capi

    n, topn = a.rows, a.topn
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    priors = rng.random(n, dtype=np.float32)
    lists = [rng.choice(n, size=1, replace=False) for _ in range(a.calls * a.regions)]
    meta = [k for k in build.kernel_metadata() if "playlist_scan_kernel" in k["name"]][0]
    out = {"rows": n, "topn": topn, "k": 1, "device": torch.cuda.get_device_name(0),
           "playlist_scan_kernel": {"vgpr": meta["vgpr"], "sgpr": meta["sgpr"], "lds": meta["lds"], "scratch": meta["scratch"]},
           "bytes_per_row": {"cosine": 12, "cosine_prior": 16, "distance": 16, "distance_no_replica": 48}}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        eng.set_priors(priors)
        cases = {"cosine": lambda rows: eng.query_playlist_topn(rows, topn),
                 "cosine_prior": lambda rows: eng.query_playlist_topn(rows, topn, prior_weight=0.25),
                 "distance": lambda rows: eng.query_nearest_rows(rows, topn)}
        out["replica"] = measure(eng, cases, lists, a.regions, a.calls)
    r = out["replica"]
    r["distance"]["ratio_to_cosine_prior"] = round(r["distance"]["call_us_median_of_regions"] / r["cosine_prior"]["call_us_median_of_regions"], 3)
    r["distance"]["ratio_to_cosine"] = round(r["distance"]["call_us_median_of_regions"] / r["cosine"]["call_us_median_of_regions"], 3)
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA) as eng:
        out["no_replica"] = measure(eng, {"distance": lambda rows: eng.query_nearest_rows(rows, topn)}, lists, a.regions, max(a.calls // 4, 5))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
