"""Diversified top-N at 10 M x 12, one handle, synchronous calls: p50 / p99 of
mi355rec_query_playlist_topn_diverse (K = 1 and K = 10, lambda = 0.7) at top-10 and top-100, with a pool of 4 x topn and a
pool of 1024, beside the _weighted call of the same members at topn = pool — the stage the re-rank sits behind — so that
(diverse p50 - weighted p50) is what the re-rank adds to a call.  The rerank kernel's own time comes from a trace:

    python tools/run_diverse.py --out profiles/r10_diverse.json [--ab path/to/parent/libmi355rec.so]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_diverse -o diverse -- python tools/run_diverse.py --profile CASE

--ab LIB: the _weighted calls at topn = pool also with LIB (the parent commit's build), in child processes alternating this,
parent, this, parent ... (--rounds each), same box, one run.  --profile CASE (e.g. top100_pool400): 200 diverse calls of that
case alone, for the trace; --kernel-stats DIR... collects the mmr_rerank_kernel rows of such traces into one CSV.
Prints one JSON document and writes it to --out."""
import argparse
import csv
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tools.run_filter import catalogue, timed  # noqa: E402

LAMBDA = 0.7
CASES = {"top10_pool40": (10, 40), "top10_pool1024": (10, 1024), "top100_pool400": (100, 400), "top100_pool1024": (100, 1024)}


def weighted_only(a):
    """One child of --ab: the weighted K = 1 / K = 10 calls at topn = pool with whichever library MI355REC_LIB names."""
    from spotify_recommender_amd import CosineEngine
    rng = np.random.default_rng(7)
    data = catalogue(a.rows)
    res = {}
    with CosineEngine(data) as eng:
        for k in (1, 10):
            lists = [rng.choice(a.rows, size=k, replace=False) for _ in range(a.calls)]
            w = np.ones(k, np.float32)
            for pool in sorted({p for _, p in CASES.values()}):
                res[f"k{k}_top{pool}"] = timed(lambda rows: eng.query_playlist_topn(rows, pool, weights=w), lists)["p50_us"]
    print("AB " + json.dumps(res))


def ab(a):
    env_b = dict(os.environ)
    env_a = dict(os.environ, MI355REC_LIB=str(Path(a.ab).resolve()), MI355REC_CAPI_LENIENT="1")
    cmd = [sys.executable, __file__, "--weighted-only", "--rows", str(a.rows), "--calls", str(a.calls)]
    runs = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for name, env in (("this", env_b), ("parent", env_a)):
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"A/B child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {"rounds": a.rounds, "order": "this, parent, this, parent, ...", "runs": runs}
    for key in runs["this"][0]:
        b = float(np.median([r[key] for r in runs["this"]]))
        p = float(np.median([r[key] for r in runs["parent"]]))
        out[f"{key}_p50_us"] = {"this": round(b, 1), "parent": round(p, 1), "ratio": round(b / p, 3)}
    return out


def kernel_stats(dirs, out_csv):
    """The mmr_rerank_kernel (and, for scale, playlist_scan_kernel / merge_kernel) rows of rocprofv3 --stats outputs."""
    rows = []
    for d in dirs:
        for f in sorted(Path(d).rglob("*kernel_stats.csv")):
            for r in csv.DictReader(f.open()):
                if any(n in r["Name"] for n in ("mmr_rerank_kernel", "playlist_scan_kernel", "merge_kernel")):
                    rows.append({"case": Path(d).name, "kernel": r["Name"].split("(")[0], "calls": r["Calls"],
                                 "average_ns": r["AverageNs"], "min_ns": r["MinNs"], "max_ns": r["MaxNs"]})
    with open(out_csv, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=["case", "kernel", "calls", "average_ns", "min_ns", "max_ns"])
        w.writeheader()
        w.writerows(rows)
    print(f"{len(rows)} rows -> {out_csv}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--profile", default="")
    ap.add_argument("--ab", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--weighted-only", action="store_true")
    ap.add_argument("--kernel-stats", nargs="+", default=[])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    if a.weighted_only:
        return weighted_only(a)
    import torch
    from spotify_recommender_amd import CosineEngine

    n = a.rows
    rng = np.random.default_rng(7)
    data = catalogue(n)
    out = {"rows": n, "lambda": LAMBDA, "calls": a.calls, "device": torch.cuda.get_device_name(0), "cases": {}}
    with CosineEngine(data) as eng:
        if a.profile:
            topn, pool = CASES[a.profile]
            lists = [rng.choice(n, size=1, replace=False) for _ in range(200)]
            print(json.dumps(timed(lambda rows: eng.query_playlist_topn_diverse(rows, topn, LAMBDA, pool), lists)))
            return
        for k in (1, 10):
            lists = [rng.choice(n, size=k, replace=False) for _ in range(a.calls)]
            w = np.ones(k, np.float32)
            for name, (topn, pool) in CASES.items():
                d = timed(lambda rows: eng.query_playlist_topn_diverse(rows, topn, LAMBDA, pool), lists)
                s = timed(lambda rows: eng.query_playlist_topn(rows, pool, weights=w), lists)
                t = timed(lambda rows: eng.query_playlist_topn(rows, topn, weights=w), lists)
                out["cases"][f"k{k}_{name}"] = {"diverse": d, "weighted_at_topn_eq_pool": s, "weighted_at_topn": t,
                                                "rerank_adds_p50_us": round(d["p50_us"] - s["p50_us"], 1),
                                                "ratio_to_weighted_at_pool_p50": round(d["p50_us"] / s["p50_us"], 3)}
    del data
    torch.cuda.empty_cache()
    if a.ab:
        out["ab_weighted_at_pool_vs_parent"] = ab(a)
        for k in (1, 10):
            for name, (topn, pool) in CASES.items():
                c = out["cases"][f"k{k}_{name}"]
                parent = out["ab_weighted_at_pool_vs_parent"][f"k{k}_top{pool}_p50_us"]["parent"]
                c["parent_weighted_at_pool_p50_us"] = parent
                c["rerank_costs_more_than_the_parents_weighted_call"] = bool(c["rerank_adds_p50_us"] > parent)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
