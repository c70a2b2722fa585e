"""Group caps at 10 M x 12, one handle, synchronous calls: groups row // 5, max_per_group 2, top-10 and
top-100, the default pool (8 x topn) and a pool of 1024, K = 1 by row.  Two questions:

(a) lambda = 1 (the loop-free path of mmr_rerank_kernel): p50 / p99 of mi355rec_query_playlist_topn_capped beside this
    tree's _weighted call of the same members at topn = pool — the capped call is that call plus one re-rank launch.
(b) lambda = 0.7 (the serial loop with the cap): the capped call beside the _diverse call with the same arguments, each in
    five repeated regions (p50 per region, their spread); with --ab LIB the _diverse regions also run against LIB (the parent
    commit's build) in child processes alternating this, parent, this, parent ..., same box, one run.

    python tools/run_capped.py --out profiles/r11_capped.json [--ab path/to/parent/libmi355rec.so]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_capped -o capped -- python tools/run_capped.py --profile CASE
    python tools/run_capped.py --kernel-stats prof_capped/... --out profiles/r11_capped_kernel_stats.csv

--profile CASE (e.g. top100_pool800): 200 capped lambda = 1 calls of that case alone, for the trace (add --lam 0.7 for the
serial loop).  Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tools.run_diverse import kernel_stats  # noqa: E402
from tools.run_filter import catalogue, timed  # noqa: E402

LAMBDA = 0.7
M = 2
REGIONS = 5
CASES = {"top10_pool80": (10, 80), "top10_pool1024": (10, 1024), "top100_pool800": (100, 800), "top100_pool1024": (100, 1024)}


def regions(call, lists):
    """p50 of each of REGIONS repeated regions over the same calls, and their spread."""
    p50 = [timed(call, lists)["p50_us"] for _ in range(REGIONS)]
    return {"p50_us_regions": [round(x, 1) for x in p50], "p50_us": round(float(np.median(p50)), 1),
            "spread_us": round(max(p50) - min(p50), 1)}


def diverse_only(a):
    """One child of --ab: the _diverse regions (lambda 0.7) with whichever library MI355REC_LIB names."""
    from spotify_recommender_amd import CosineEngine
    rng = np.random.default_rng(7)
    data = catalogue(a.rows)
    res = {}
    with CosineEngine(data) as eng:
        lists = [rng.choice(a.rows, size=1, replace=False) for _ in range(a.calls)]
        for name, (topn, pool) in CASES.items():
            res[name] = regions(lambda rows: eng.query_playlist_topn_diverse(rows, topn, LAMBDA, pool), lists)
    print("AB " + json.dumps(res))


def ab(a):
    env_b = dict(os.environ)
    env_a = dict(os.environ, MI355REC_LIB=str(Path(a.ab).resolve()), MI355REC_CAPI_LENIENT="1")
    cmd = [sys.executable, __file__, "--diverse-only", "--rows", str(a.rows), "--calls", str(a.calls)]
    runs = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for name, env in (("this", env_b), ("parent", env_a)):
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"A/B child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {"rounds": a.rounds, "order": "this, parent, this, parent, ...", "runs": runs}
    for key in CASES:
        b = [x for r in runs["this"] for x in r[key]["p50_us_regions"]]
        p = [x for r in runs["parent"] for x in r[key]["p50_us_regions"]]
        out[f"{key}_diverse_p50_us"] = {"this": round(float(np.median(b)), 1), "parent": round(float(np.median(p)), 1),
                                        "this_spread": round(max(b) - min(b), 1), "parent_spread": round(max(p) - min(p), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--profile", default="")
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--ab", default="")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--diverse-only", action="store_true")
    ap.add_argument("--kernel-stats", nargs="+", default=[])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    if a.diverse_only:
        return diverse_only(a)
    import torch
    from spotify_recommender_amd import CosineEngine

    n = a.rows
    rng = np.random.default_rng(7)
    data = catalogue(n)
    groups = (np.arange(n, dtype=np.int64) // 5).astype(np.int32)
    out = {"rows": n, "groups": "row // 5", "max_per_group": M, "lambda_serial": LAMBDA, "calls": a.calls, "regions": REGIONS,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    with CosineEngine(data) as eng:
        eng.set_groups(groups)
        if a.profile:
            topn, pool = CASES[a.profile]
            lists = [rng.choice(n, size=1, replace=False) for _ in range(200)]
            print(json.dumps(timed(lambda rows: eng.query_playlist_topn_capped(rows, topn, M, a.lam, pool), lists)))
            return
        lists = [rng.choice(n, size=1, replace=False) for _ in range(a.calls)]
        w = np.ones(1, np.float32)
        for name, (topn, pool) in CASES.items():
            par = timed(lambda rows: eng.query_playlist_topn_capped(rows, topn, M, 1.0, pool), lists)
            wt = timed(lambda rows: eng.query_playlist_topn(rows, pool, weights=w), lists)
            ser = regions(lambda rows: eng.query_playlist_topn_capped(rows, topn, M, LAMBDA, pool), lists)
            div = regions(lambda rows: eng.query_playlist_topn_diverse(rows, topn, LAMBDA, pool), lists)
            out["cases"][name] = {"a_capped_lambda1": par, "a_weighted_at_topn_eq_pool": wt,
                                  "a_rerank_adds_p50_us": round(par["p50_us"] - wt["p50_us"], 1),
                                  "b_capped_lambda07": ser, "b_diverse_lambda07_this_tree": div,
                                  "b_capped_minus_diverse_p50_us": round(ser["p50_us"] - div["p50_us"], 1)}
    del data
    torch.cuda.empty_cache()
    if a.ab:
        out["ab_diverse_vs_parent"] = ab(a)
        for name in CASES:
            c = out["cases"][name]
            parent = out["ab_diverse_vs_parent"][f"{name}_diverse_p50_us"]
            c["b_parent_diverse_p50_us"] = parent["parent"]
            c["b_capped_minus_parent_diverse_p50_us"] = round(c["b_capped_lambda07"]["p50_us"] - parent["parent"], 1)
            c["b_within_spread"] = bool(abs(c["b_capped_minus_parent_diverse_p50_us"])
                                        <= max(parent["parent_spread"], c["b_capped_lambda07"]["spread_us"]))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
