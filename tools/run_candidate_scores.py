"""CANDIDATE SCORES at 10 M x 12, one handle with the 8-bit replica, synchronous calls (include/mi355rec_diag.h, CANDIDATE SCORES;
DESIGN.md 5.4.16).  In one process, on one handle over uniform random rows, K = 1 by row, for ascending random lists of 100 ...
1 000 000 ids, the kinds
    scores                 engine.candidate_scores on the list (the gather launch in score mode, 8 B per entry copied back, no merge)
    topn_100               the _candidates top-100 call on the same list (the gather launch, the merge, 100 results)
alternate pass by pass (a pass = --calls synchronous calls; its p50 is kept).  Per kind: the median, minimum and maximum of the
passes' p50.

    python tools/run_candidate_scores.py --out profiles/r21_candidate_scores.json

--ab LIB: the A/B against another build of the library (the parent commit's): requests without a list (tools/playlist_ab.py's
plain_k1 and plain_k10) and _candidates top-100 requests on ascending lists of 1 000 and 100 000 ids, in ALTERNATING child processes
(this tree, LIB, this tree, ...), --rounds children a side.  Per kind: each side's median p50, the parent's minimum and maximum, and
whether this tree's median lies within them (or below).

    python tools/run_candidate_scores.py --ab path/to/parent/libmi355rec.so --out profiles/r21_candidate_scores_ab.json"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from playlist_ab import kinds_of, p50_us  # noqa: E402
from run_candidates import SIZES, measure  # noqa: E402

AB_LISTS = (1_000, 100_000)


def main_measure(a):
    import torch
    from spotify_recommender_amd import CosineEngine, build, capi
    from spotify_recommender_amd.engine import candidate_scores, with_candidates

    n, topn = a.rows, 100
    rng = np.random.default_rng(21)
    feats = rng.random((n, 12), dtype=np.float32)
    meta = [k for k in build.kernel_metadata() if "playlist_scan_kernel" in k["name"]][0]
    out = {"rows": n, "topn": topn, "k": 1, "members": "by row", "replica": "on", "device": torch.cuda.get_device_name(0),
           "playlist_scan_kernel": {"vgpr": meta["vgpr"], "sgpr": meta["sgpr"], "lds": meta["lds"], "scratch": meta["scratch"]}, "sizes": {}}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        rows = np.asarray([0], np.int64)
        for size in SIZES:
            if size > n:
                continue
            ids = np.sort(rng.choice(n, size=size, replace=False)).astype(np.int64)
            view = with_candidates(eng, ids)
            calls = min(a.calls, max(10, 2_000_000 // size))
            r = measure({"scores": (lambda ids=ids: candidate_scores(eng, ids, rows=rows), calls),
                         "topn_100": (lambda view=view: view.query_playlist_topn(rows, topn), calls)}, a.passes)
            r["scores_over_topn_100"] = round(r["scores"]["p50_us_median_of_passes"] / r["topn_100"]["p50_us_median_of_passes"], 3)
            out["sizes"][str(size)] = r
    out["scores_no_slower_than_topn_100"] = all(r["scores_over_topn_100"] <= 1.0 for r in out["sizes"].values())
    return out


def child(a):
    """One A/B child: the kinds with whichever library MI355REC_LIB names (none: this tree's)."""
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import with_candidates
    n = a.rows
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    res = {}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        table = kinds_of(eng, 100)
        for kind in ("plain_k1", "plain_k10"):
            k, call = table[kind]
            res[kind] = p50_us(call, [rng.choice(n, size=k, replace=False) for _ in range(a.calls)])
        for size in AB_LISTS:
            view = with_candidates(eng, np.sort(rng.choice(n, size=size, replace=False)).astype(np.int64))
            res[f"candidates_{size}_top100"] = p50_us(lambda rows: view.query_playlist_topn(rows, 100),
                                                      [rng.choice(n, size=1, replace=False) for _ in range(a.calls)])
    print("AB " + json.dumps(res))


def main_ab(a):
    env_this = dict(os.environ)
    env_this.pop("MI355REC_LIB", None)
    env_parent = dict(os.environ, MI355REC_LIB=str(Path(a.ab).resolve()), MI355REC_CAPI_LENIENT="1")
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--rows", str(a.rows), "--calls", str(a.calls)]
    runs = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for name, env in (("this", env_this), ("parent", env_parent)):
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"A/B child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {"rows": a.rows, "topn": 100, "calls": a.calls, "rounds": a.rounds, "order": "this, parent, this, parent, ...", "runs": runs}
    for kind in runs["this"][0]:
        mine, theirs = [r[kind] for r in runs["this"]], [r[kind] for r in runs["parent"]]
        out[f"{kind}_p50_us"] = {"this": round(float(np.median(mine)), 1), "parent": round(float(np.median(theirs)), 1),
                                 "parent_min": min(theirs), "parent_max": max(theirs),
                                 "ratio": round(float(np.median(mine)) / float(np.median(theirs)), 3),
                                 "within_parent_min_max": bool(float(np.median(mine)) <= max(theirs))}
    out["all_within_parent_min_max"] = all(out[f"{kind}_p50_us"]["within_parent_min_max"] for kind in runs["this"][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=100, help="calls per pass (A/B: per kind and child)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="A/B: children per library")
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit: run the A/B instead")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    text = json.dumps(main_ab(a) if a.ab else main_measure(a), indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
