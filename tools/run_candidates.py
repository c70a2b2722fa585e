"""CANDIDATE LISTS at 10 M x 12, top-100, one handle with the 8-bit replica, synchronous calls (include/mi355rec_diag.h, CANDIDATE
LISTS).  In one process, on one handle over uniform random rows, members by row, for K = 1 and K = 10 and both
metrics, and for random lists of 100 ... 1 000 000 ids handed over once ascending and once shuffled, the kinds
    gather                 the request with the list (the gather launch)
    only_premade           the same request with an ONLY RowSet made beforehand from the same ids (one pass over the catalogue)
    only_per_request       ... with the ONLY set made, uploaded and destroyed per request (what a per-request list costs without the
                           gather: only= given a plain id array)
    plain                  the request without list or set, for scale
alternate pass by pass (a pass = --calls synchronous calls, each ending in the host's wait for the result; its p50 is kept).  Per kind:
the median, minimum and maximum of the passes' p50.  The host's share is reported apart: host_pass_us is a request whose list names
no row of the handle (the checks and the one pass over the list, then no launch), and shuffled minus ascending is the sort.
crossover: per K and metric, the smallest measured list size at which gather's median is no longer below only_premade's.

    python tools/run_candidates.py --out profiles/r19_candidates.json"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SIZES = (100, 1_000, 10_000, 100_000, 1_000_000)


def pass_p50_us(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.percentile(np.asarray(ts) * 1e6, 50))


def measure(cases, passes):
    """{name: figures}; cases = {name: (fn, calls per pass)}: the cases alternate pass by pass."""
    for fn, _ in cases.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in cases}
    for _ in range(passes):
        for name, (fn, calls) in cases.items():
            times[name].append(pass_p50_us(fn, calls))
    return {name: {"p50_us_median_of_passes": round(float(np.median(ts)), 1), "p50_us_min": round(float(np.min(ts)), 1),
                   "p50_us_max": round(float(np.max(ts)), 1), "passes": passes, "calls_per_pass": cases[name][1]}
            for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=100, help="calls per pass")
    ap.add_argument("--slow-calls", type=int, default=20, help="calls per pass of only_per_request")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from spotify_recommender_amd import CosineEngine, build, capi
    from spotify_recommender_amd.engine import candidates_counters, with_candidates

    n, topn = a.rows, a.topn
    rng = np.random.default_rng(19)
    feats = rng.random((n, 12), dtype=np.float32)
    meta = [k for k in build.kernel_metadata() if "playlist_scan_kernel" in k["name"]][0]
    out = {"rows": n, "topn": topn, "device": torch.cuda.get_device_name(0),
           "playlist_scan_kernel": {"vgpr": meta["vgpr"], "sgpr": meta["sgpr"], "lds": meta["lds"], "scratch": meta["scratch"]},
           "kinds": {}, "crossover": {}}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        for k in (1, 10):
            rows = np.concatenate([[0], rng.choice(np.arange(1, n), size=k - 1, replace=False)]).astype(np.int64)
            for metric in ("cosine", "distance"):
                def call(e, metric=metric, rows=rows, **kw):
                    if metric == "cosine":
                        return e.query_playlist_topn(rows, topn, **kw)
                    return e.query_nearest_rows_scaled(rows, topn, None, **kw)
                res = {}
                for size in SIZES:
                    if size > n:
                        continue
                    ids = np.sort(rng.choice(n, size=size, replace=False)).astype(np.int64)
                    shuffled = rng.permutation(ids)
                    outside = np.arange(n, n + size, dtype=np.int64)
                    calls = min(a.calls, max(10, 2_000_000 // size))     # (a shuffled list of 10^6 ids is sorted per call: tens of ms)
                    with eng.row_set(ids) as premade:
                        for order, handed in (("ascending", ids), ("shuffled", shuffled)):
                            view, nothing = with_candidates(eng, handed), with_candidates(eng, outside if order == "ascending" else outside[::-1].copy())
                            cases = {
                                "gather": (lambda view=view: call(view), calls),
                                "only_premade": (lambda s=premade: call(eng, only=s), a.calls),
                                "only_per_request": (lambda handed=handed: call(eng, only=handed), min(a.slow_calls, calls)),
                                "plain": (lambda: call(eng), a.calls),
                                "host_pass": (lambda nothing=nothing: call(nothing), calls),   # (ids of no row: the checks and the pass, no launch)
                            }
                            before = candidates_counters(eng)
                            r = measure(cases, a.passes)
                            after = candidates_counters(eng)
                            launches = after["requests"] - before["requests"]
                            r["rows_gathered_per_request"] = (after["rows_gathered"] - before["rows_gathered"]) // max(launches, 1)
                            r["host_pass_us"] = r.pop("host_pass")["p50_us_median_of_passes"]
                            res[f"{size}_{order}"] = r
                    res[f"{size}_sort_us"] = round(res[f"{size}_shuffled"]["gather"]["p50_us_median_of_passes"] -
                                                   res[f"{size}_ascending"]["gather"]["p50_us_median_of_passes"], 1)
                name = f"{metric}_k{k}"
                out["kinds"][name] = res
                lost = [size for size in SIZES if f"{size}_ascending" in res and
                        res[f"{size}_ascending"]["gather"]["p50_us_median_of_passes"] >= res[f"{size}_ascending"]["only_premade"]["p50_us_median_of_passes"]]
                out["crossover"][name] = {"gather_stops_winning_at": lost[0] if lost else None, "largest_size_measured": max(s for s in SIZES if s <= n)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
