"""FEATURE SCALES at 10 M x 12, top-100, one handle, synchronous calls (include/mi355rec_diag.h, FEATURE SCALES),
by the protocol of tools/run_distance.py: in one process, on one handle over uniform random rows, members by row, the cases
    cosine_k1 / cosine_k10                  the cosine playlist request without scales (12 B per row over the 8-bit replica);
    cosine_drop3_k1 / _k10                  the same with key, mode and the genre id at 0 (the per-row cut of the scaled pre-filter);
    cosine_general_k1 / _k10                the same with the scales [2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0];
    distance_k1                             the distance request without scales (12 + 4 B per row, its own pre-filter);
    distance_drop3_k1 / distance_drop3_k10  the scaled distance request: the exact path, every row takes the chains
alternate region by region (a region = --calls synchronous calls, each ending in the host's wait for the result); per case the
median over the regions of the region's mean call time, the spread of the regions, the scan kernel's time (HIP events:
mi355rec_set_timing, a run of its own) and the rows whose chains were computed per query (mi355rec_playlist_counters).

--ab PARENT_LIB: calls without scales must not pay for the branch.  The three cases of tools/run_distance.py (cosine,
cosine_prior, distance; K = 1) run in child processes that alternate between this tree's library and the parent commit's
(MI355REC_LIB), --rounds each; per case every region of every child is kept, and this tree's median is compared with the parent's
median times the parent's own spread (max over min of its regions).
Prints one JSON document and writes it to --out.

    python tools/run_scaled.py --ab path/to/parent/libmi355rec.so --out profiles/r15_scaled.json"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tools.run_distance import kernel_us, region  # noqa: E402

DROP3 = [1, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 0]
GENERAL = [2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0]


def measure(eng, cases, regions, calls):
    """{name: figures}; cases = {name: (fn, member lists)}: the cases alternate region by region."""
    for fn, lists in cases.values():           # warm-up: every shape the timed regions use (and the norms' build)
        for x in lists[:10]:
            fn(x)
    times = {name: [] for name in cases}
    for r in range(regions):
        for name, (fn, lists) in cases.items():
            times[name].append(region(fn, lists[r * calls:(r + 1) * calls]))
    out = {}
    for name, (fn, lists) in cases.items():
        ts = np.asarray(times[name])
        before = eng.playlist_counters()
        k_us = kernel_us(eng, fn, lists[:20])
        after = eng.playlist_counters()
        out[name] = {"call_us_median_of_regions": round(float(np.median(ts)), 1), "call_us_min": round(float(ts.min()), 1),
                     "call_us_max": round(float(ts.max()), 1), "regions": regions, "calls_per_region": calls,
                     "playlist_scan_kernel_us": k_us, "rows_exact_per_query": (after["rows_exact"] - before["rows_exact"]) // 20}
    return out


def unscaled_only(a):
    """One child of --ab: run_distance's three cases with whichever library MI355REC_LIB names; every region's time."""
    from spotify_recommender_amd import CosineEngine, capi
    n, topn = a.rows, a.topn
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    priors = rng.random(n, dtype=np.float32)
    lists = [rng.choice(n, size=1, replace=False) for _ in range(a.calls * a.regions)]
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        eng.set_priors(priors)
        cases = {"cosine": lambda rows: eng.query_playlist_topn(rows, topn),
                 "cosine_prior": lambda rows: eng.query_playlist_topn(rows, topn, prior_weight=0.25),
                 "distance": lambda rows: eng.query_nearest_rows(rows, topn)}
        for fn in cases.values():
            for x in lists[:20]:
                fn(x)
        times = {name: [] for name in cases}
        for r in range(a.regions):
            for name, fn in cases.items():
                times[name].append(round(region(fn, lists[r * a.calls:(r + 1) * a.calls]), 2))
    print("AB " + json.dumps(times))


def ab(a):
    env_b = dict(os.environ)
    env_a = dict(os.environ, MI355REC_LIB=str(Path(a.ab).resolve()), MI355REC_CAPI_LENIENT="1")
    cmd = [sys.executable, __file__, "--unscaled-only", "--rows", str(a.rows), "--calls", str(a.calls), "--regions", str(a.regions),
           "--topn", str(a.topn)]
    runs = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for name, env in (("parent", env_a), ("this", env_b)):
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"A/B child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {"rounds": a.rounds, "order": "parent, this, parent, this, ...", "regions_per_child": a.regions, "calls_per_region": a.calls,
           "region_call_us": runs}
    for case in ("cosine", "cosine_prior", "distance"):
        mine = [t for r in runs["this"] for t in r[case]]
        theirs = [t for r in runs["parent"] for t in r[case]]
        b, p, spread = float(np.median(mine)), float(np.median(theirs)), max(theirs) / min(theirs)
        out[case] = {"this_median_us": round(b, 1), "parent_median_us": round(p, 1), "ratio": round(b / p, 4),
                     "parent_max_over_min": round(spread, 4), "within_parent_spread": bool(b <= p * spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed region")
    ap.add_argument("--regions", type=int, default=7, help="timed regions per case (at least 5)")
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3, help="--ab: children per library")
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit")
    ap.add_argument("--unscaled-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions: at least 5")
    if a.unscaled_only:
        return unscaled_only(a)
    import torch
    from spotify_recommender_amd import CosineEngine, build, capi

    n, topn = a.rows, a.topn
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    lists = {k: [rng.choice(n, size=k, replace=False) for _ in range(a.calls * a.regions)] for k in (1, 10)}
    meta = [k for k in build.kernel_metadata() if "playlist_scan_kernel" in k["name"]][0]
    out = {"rows": n, "topn": topn, "device": torch.cuda.get_device_name(0),
           "playlist_scan_kernel": {"vgpr": meta["vgpr"], "sgpr": meta["sgpr"], "lds": meta["lds"], "scratch": meta["scratch"]},
           "scales": {"drop3": DROP3, "general": GENERAL}}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        cases = {}
        for k in (1, 10):
            cases[f"cosine_k{k}"] = (lambda rows: eng.query_playlist_topn(rows, topn), lists[k])
            cases[f"cosine_drop3_k{k}"] = (lambda rows: eng.query_playlist_topn(rows, topn, scales=DROP3), lists[k])
            cases[f"cosine_general_k{k}"] = (lambda rows: eng.query_playlist_topn(rows, topn, scales=GENERAL), lists[k])
        cases["distance_k1"] = (lambda rows: eng.query_nearest_rows(rows, topn), lists[1])
        cases["distance_drop3_k1"] = (lambda rows: eng.query_nearest_rows_scaled(rows, topn, DROP3), lists[1])
        cases["distance_drop3_k10"] = (lambda rows: eng.query_nearest_rows_scaled(rows, topn, DROP3), lists[10])
        out["replica"] = measure(eng, cases, a.regions, a.calls)
    if a.ab:
        out["unscaled_vs_parent"] = ab(a)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
