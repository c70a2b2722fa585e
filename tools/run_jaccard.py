"""JACCARD REQUESTS at 10 M x 12, one handle, synchronous calls, top-100, members by row (include/mi355rec_diag.h, JACCARD
REQUESTS).  In one process, for K = 1, 3, 10, 32 the kinds
    jaccard                the Jaccard request
    cosine                 the playlist request (the plain mean) with the same members
    distance               the distance request with the same members
    manhattan              the Manhattan request with the same members
alternate pass by pass (a pass = --calls synchronous calls with fresh members; its p50 is kept), once on a handle with the 8-bit
replica ("replica_on": the other kinds' pre-filters; the Jaccard request has none and takes the chains on every row) and once on a
handle that never built one ("replica_off": every row takes the chains for every kind).  Per kind: the median, minimum and
maximum of the passes' p50, and rows_exact per call (mi355rec_playlist_counters).  Uniform random rows.  The protocol is
tools/run_manhattan.py's.

    python tools/run_jaccard.py --out profiles/r27_jaccard.json

--ab LIB: the A/B against another build of the library (the parent commit's), because playlist_scan_kernel's code changed:
tools/playlist_ab.py's plain_k1, distance_k1, prior_k10 and bounded_count_k1 in ALTERNATING child processes, --rounds children a
side; each ratio beside the parent's own spread over its children.

    python tools/run_jaccard.py --ab path/to/parent/libmi355rec.so --out profiles/r27_jaccard_ab.json"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from playlist_ab import run  # noqa: E402
from run_anyof import pass_p50_us  # noqa: E402

KS = (1, 3, 10, 32)
AB_KINDS = ("plain_k1", "distance_k1", "prior_k10", "bounded_count_k1")


def measure_catalogue(eng, n, a, topn):
    from spotify_recommender_amd.engine import query_jaccard, query_manhattan
    rng = np.random.default_rng(27)
    out = {}
    for k in KS:
        kinds = {"jaccard": lambda rows: query_jaccard(eng, topn, rows=rows), "cosine": lambda rows: eng.query_playlist_topn(rows, topn),
                 "distance": lambda rows: eng.query_nearest_rows(rows, topn), "manhattan": lambda rows: query_manhattan(eng, topn, rows=rows)}
        times = {name: [] for name in kinds}
        exact = {}
        for fn in kinds.values():
            for _ in range(3):
                fn(np.ascontiguousarray(rng.choice(n, size=k, replace=False).astype(np.int64)))
        for _ in range(a.passes):
            for name, fn in kinds.items():
                lists = [np.ascontiguousarray(rng.choice(n, size=k, replace=False).astype(np.int64)) for _ in range(a.calls)]
                before = eng.playlist_counters()["rows_exact"]
                times[name].append(pass_p50_us(fn, lists))
                exact.setdefault(name, []).append((eng.playlist_counters()["rows_exact"] - before) / a.calls)
        out[f"k{k}"] = {name: {"p50_us_median_of_passes": round(float(np.median(ts)), 1), "p50_us_min": round(float(np.min(ts)), 1),
                               "p50_us_max": round(float(np.max(ts)), 1), "rows_exact_per_call": round(float(np.median(exact[name])), 1)}
                        for name, ts in times.items()}
        r = out[f"k{k}"]
        print(f"K = {k}: " + ", ".join(f"{name} {r[name]['p50_us_median_of_passes']} us ({r[name]['rows_exact_per_call']} rows exact)"
                                        for name in kinds), file=sys.stderr, flush=True)
    return out


def both_modes(make_feats, n, a, topn):
    from spotify_recommender_amd import CosineEngine, capi
    out = {}
    for mode in ("replica_on", "replica_off"):
        feats = make_feats()
        with CosineEngine(feats, flags=0 if mode == "replica_on" else capi.CREATE_NO_REPLICA) as eng:
            if mode == "replica_on":
                eng.set_replica(capi.REPLICA_ON)
            print(f"[{mode}]", file=sys.stderr, flush=True)
            out[mode] = measure_catalogue(eng, n, a, topn)
        del feats
    out["jaccard_on_over_off"] = {f"k{k}": round(out["replica_on"][f"k{k}"]["jaccard"]["p50_us_median_of_passes"] /
                                                 out["replica_off"][f"k{k}"]["jaccard"]["p50_us_median_of_passes"], 3) for k in KS}
    return out


def main_measure(a):
    import torch
    from spotify_recommender_amd import build

    n, topn = a.rows, 100
    meta = {f: [k for k in build.kernel_metadata() if f in k["name"]][0] for f in ("anyof_scan_kernel", "manhattan_scan_kernel", "playlist_scan_kernel")}
    out = {"rows": n, "topn": topn, "members": "by row", "device": torch.cuda.get_device_name(0), "passes": a.passes,
           "calls_per_pass": a.calls, "library": os.environ.get("MI355REC_LIB", "the tree's product library"), "prefilter": "none",
           "kernels": {f: {x: m[x] for x in ("vgpr", "sgpr", "lds", "scratch")} for f, m in meta.items()}}
    out["uniform"] = both_modes(lambda: np.random.default_rng(21).random((n, 12), dtype=np.float32), n, a, topn)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=40, help="calls per pass (A/B: per kind and child)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="A/B: children per library")
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit: run the A/B instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    doc = run(a.ab, a.rows, a.calls, 100, a.rounds, AB_KINDS) if a.ab else main_measure(a)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
