"""A/B of the playlist request family against another build of the library (the parent commit's, as a rule): this tree's
library and LIB in ALTERNATING child processes, the same seeded catalogue and requests in each, one p50 per kind of request and
child.  Per kind: the median p50 of each side, their ratio, and the parent's own spread (max - min over its median) — a ratio
inside that spread says nothing; add rounds.  The kinds cover every cut of the pre-filter (csrc/playlist_cut.hip.h) and the
label and filter tests:

    plain_k1, plain_k10      the cosine request, nothing else asked
    prior_k10                with a uniform row prior, beta = 0.25
    distance_k1, _k10        the distance request
    scaled_k10               cosine with the scale set [2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0]
    labelled_k10             within 3 of 114 labels (uniformly dealt)
    filtered_k10             one feature within [0, 0.1]: about 10 % of the rows pass
    anyof_k1, _k10, _k32     the any-of request (engine.query_anyof: with out_member)
    bounded_count_k1         the bounded request, count only (engine.query_bounded, topn = 0) at the cosine floor 0.97
    manhattan_k1, _k10       the Manhattan request (engine.query_manhattan: manhattan_scan_kernel)
    jaccard_k1               the Jaccard request (engine.query_jaccard: no pre-filter, every row takes the chain)
    candidates_k1            the cosine request within a fixed ascending list of 100 000 ids (engine.with_candidates: the gather)

    python tools/playlist_ab.py --ab path/to/parent/libmi355rec.so [--kinds plain_k1,prior_k10] --out profiles/r16_playlist_cut_ab.json

tools/run_filter.py, run_weighted.py and run_prior.py call run() for their own --ab (the plain kinds: the path their features
must not slow down)."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

GENERAL = [2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0]
N_LABELS = 114
N_LISTED = 100_000
PLAIN = ("plain_k1", "plain_k10")


def kinds_of(eng, topn):
    """{kind: (K, call)}; a kind that needs side data loads it on first use."""
    from spotify_recommender_amd.engine import query_anyof, query_bounded, query_jaccard, query_manhattan, with_candidates
    listed = np.arange(N_LISTED, dtype=np.int64) * ((eng.rows if eng else N_LISTED) // N_LISTED)   # ascending, spread over the catalogue
    return {
        "manhattan_k1": (1, lambda rows: query_manhattan(eng, topn, rows=rows)),
        "manhattan_k10": (10, lambda rows: query_manhattan(eng, topn, rows=rows)),
        "jaccard_k1": (1, lambda rows: query_jaccard(eng, topn, rows=rows)),
        "candidates_k1": (1, lambda rows: with_candidates(eng, listed).query_playlist_topn(rows, topn)),
        "bounded_count_k1": (1, lambda rows: query_bounded(eng, 0, 0.97, rows=rows)),
        "anyof_k1": (1, lambda rows: query_anyof(eng, topn, rows=rows)),
        "anyof_k10": (10, lambda rows: query_anyof(eng, topn, rows=rows)),
        "anyof_k32": (32, lambda rows: query_anyof(eng, topn, rows=rows)),
        "plain_k1": (1, lambda rows: eng.query_playlist_topn(rows, topn)),
        "plain_k10": (10, lambda rows: eng.query_playlist_topn(rows, topn)),
        "prior_k10": (10, lambda rows: eng.query_playlist_topn(rows, topn, prior_weight=0.25)),
        "distance_k1": (1, lambda rows: eng.query_nearest_rows(rows, topn)),
        "distance_k10": (10, lambda rows: eng.query_nearest_rows(rows, topn)),
        "scaled_k10": (10, lambda rows: eng.query_playlist_topn(rows, topn, scales=GENERAL)),
        "labelled_k10": (10, lambda rows: eng.query_playlist_topn(rows, topn, labels=[5, 40, 77])),
        "filtered_k10": (10, lambda rows: eng.query_playlist_topn(rows, topn, where={3: (0.0, 0.1)})),
    }


def p50_us(fn, args, warm=20):
    for x in args[:warm]:
        fn(x)
    ts = []
    for x in args:
        t0 = time.perf_counter()
        fn(x)
        ts.append(time.perf_counter() - t0)
    return round(float(np.percentile(np.asarray(ts) * 1e6, 50)), 1)


def child(a):
    """One child: every asked kind with whichever library MI355REC_LIB names (none: this tree's)."""
    from spotify_recommender_amd import CosineEngine
    n = a.rows
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    res = {}
    with CosineEngine(feats) as eng:
        table = kinds_of(eng, a.topn)
        for kind in a.kinds.split(","):
            k, call = table[kind]
            if kind.startswith("prior"):
                eng.set_priors(np.random.default_rng(8).random(n, dtype=np.float32))
            if kind.startswith("labelled"):
                eng.set_labels(np.random.default_rng(9).integers(0, N_LABELS, size=n).astype(np.int32))
            lists = [rng.choice(n, size=k, replace=False) for _ in range(a.calls)]
            res[kind] = p50_us(call, lists)
    print("AB " + json.dumps(res))


def run(lib, rows, calls, topn, rounds, kinds=PLAIN):
    """The A/B document: `rounds` children per side, this tree first."""
    env_this = dict(os.environ)
    env_this.pop("MI355REC_LIB", None)
    env_parent = dict(os.environ, MI355REC_LIB=str(Path(lib).resolve()), MI355REC_CAPI_LENIENT="1")
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--rows", str(rows), "--calls", str(calls), "--topn", str(topn),
           "--kinds", ",".join(kinds)]
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for name, env in (("this", env_this), ("parent", env_parent)):
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"A/B child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {"rows": rows, "topn": topn, "calls": calls, "rounds": rounds, "order": "this, parent, this, parent, ...", "runs": runs}
    for kind in kinds:
        mine, theirs = [r[kind] for r in runs["this"]], [r[kind] for r in runs["parent"]]
        b, p = float(np.median(mine)), float(np.median(theirs))
        out[f"{kind}_p50_us"] = {"this": round(b, 1), "parent": round(p, 1), "ratio": round(b / p, 3),
                                 "parent_spread": round((max(theirs) - min(theirs)) / p, 3)}
    out["within_3pct"] = all(out[f"{kind}_p50_us"]["ratio"] <= 1.03 for kind in kinds)   # the project's bar for "unchanged"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3, help="children per library")
    ap.add_argument("--kinds", default=",".join(kinds_of(None, 0)), help="comma-separated, of the kinds above (default: all)")
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    unknown = [k for k in a.kinds.split(",") if k not in kinds_of(None, 0)]
    if unknown:
        raise SystemExit(f"unknown kinds {unknown}: of {', '.join(kinds_of(None, 0))}")
    if a.child:
        return child(a)
    if not a.ab:
        raise SystemExit("--ab LIB: the library to compare against")
    text = json.dumps(run(a.ab, a.rows, a.calls, a.topn, a.rounds, tuple(a.kinds.split(","))), indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
