"""BOUNDED REQUESTS at 10 M x 12, one handle with the 8-bit replica, synchronous calls, K = 1 by row (include/mi355rec_diag.h, BOUNDED
REQUESTS).  Child processes ALTERNATE between this tree's library and LIB (the parent commit's build), the same
seeded catalogue and member rows in each, one p50 per kind and child.  The kinds:

    plain_top100           the plain playlist request, top-100 (both libraries: the yardstick)
    count_tight            count only (topn = 0) at a floor that about 1 000 rows pass: the request's own 1 000th score
    count_median           count only at the median score of the catalogue for that member (taken from a 100 000-row sample)
    top100_tight           topn = 100 with the tight floor: the count launch and the seeded top-N launch
    top100_median          topn = 100 with the median floor

The floors are taken per member row BEFORE the timed calls (untimed plain and candidate-score requests).  Per kind: the median,
minimum and maximum of the children's p50 on each side, the ratio to the parent's plain_top100 and the parent's own spread
((max - min) / median of its plain_top100): a difference inside that spread says nothing.  The parent serves only plain_top100.

    python tools/run_bounded.py --ab path/to/parent/libmi355rec.so --out profiles/r25_bounded.json

The proven-in shortcut of the count launch on and off (the experiments build reads MI355REC_EXP_NO_PROVEN_IN), alternating children:

    python tools/run_bounded.py --shortcut-ab --out profiles/r26_bounded_shortcut_ab.json

The existing kinds against the parent (no kernel changed in figures, but the count branch sits in the tile loop): tools/playlist_ab.py
with the same --ab."""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from playlist_ab import p50_us  # noqa: E402

BOUNDED_KINDS = ("count_tight", "count_median", "top100_tight", "top100_median")


def child(a):
    """One child: plain_top100 and, with --bounded, the bounded kinds, with whichever library MI355REC_LIB names (none: this tree's)."""
    from spotify_recommender_amd import CosineEngine, engine
    n = a.rows
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    res, matches = {}, {}
    with CosineEngine(feats) as eng:
        lists = [rng.choice(n, size=1, replace=False) for _ in range(a.calls)]
        sample = np.sort(rng.choice(n, size=min(n, 100_000), replace=False))
        res["plain_top100"] = p50_us(lambda rows: eng.query_playlist_topn(rows, 100), lists)
        if a.bounded:
            tight = [float(eng.query_playlist_topn(rows, 1000)[1][-1]) for rows in lists]
            median = [float(np.nanmedian(engine.candidate_scores(eng, sample, rows=rows)[0])) for rows in lists]   # (NaN: the member row itself)
            for kind, topn, floors in (("count_tight", 0, tight), ("count_median", 0, median), ("top100_tight", 100, tight),
                                       ("top100_median", 100, median)):
                args = list(zip(lists, floors))
                before = eng.playlist_counters()
                res[kind] = p50_us(lambda x: engine.query_bounded(eng, topn, x[1], rows=x[0]), args)
                after = eng.playlist_counters()
                totals = [engine.query_bounded(eng, 0, f, rows=r)[2] for r, f in args[:20]]
                matches[kind] = {"median_total": float(np.median(totals)),
                                 "rows_exact_per_call": (after["rows_exact"] - before["rows_exact"]) / (len(args) + min(20, len(args)))}
    print("AB " + json.dumps({"p50_us": res, "matches": matches}))


def run(lib, rows, calls, rounds):
    env_this = dict(os.environ)
    env_this.pop("MI355REC_LIB", None)
    env_parent = dict(os.environ, MI355REC_LIB=str(Path(lib).resolve()), MI355REC_CAPI_LENIENT="1")
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--rows", str(rows), "--calls", str(calls)]
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for name, env, more in (("this", env_this, ["--bounded"]), ("parent", env_parent, [])):
            p = subprocess.run(cmd + more, env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    theirs = [r["p50_us"]["plain_top100"] for r in runs["parent"]]
    parent = float(np.median(theirs))
    out = {"rows": rows, "members": "K = 1 by row", "calls": calls, "rounds": rounds, "order": "this, parent, this, parent, ...", "runs": runs,
           "parent_plain_top100_p50_us": round(parent, 1), "parent_spread": round((max(theirs) - min(theirs)) / parent, 3)}
    for kind in ("plain_top100",) + BOUNDED_KINDS:
        mine = [r["p50_us"][kind] for r in runs["this"]]
        out[f"{kind}_p50_us"] = {"median": round(float(np.median(mine)), 1), "min": min(mine), "max": max(mine),
                                 "over_parent_plain_top100": round(float(np.median(mine)) / parent, 3)}
    return out


def run_shortcut(rows, calls, rounds):
    """The proven-in shortcut (csrc/playlist_cut.hip.h, "BOUNDED") on and off: the experiments build in alternating children, every
    other one with MI355REC_EXP_NO_PROVEN_IN set.  The totals are the same either way (each child reports them)."""
    from spotify_recommender_amd import build
    base = dict(os.environ, MI355REC_LIB=str(build.LIB_EXPERIMENTS), MI355REC_CAPI_LENIENT="1")
    base.pop("MI355REC_EXP_NO_PROVEN_IN", None)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--bounded", "--rows", str(rows), "--calls", str(calls)]
    runs = {"on": [], "off": []}
    for _ in range(rounds):
        for name, env in (("on", base), ("off", dict(base, MI355REC_EXP_NO_PROVEN_IN="1"))):
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"child (shortcut {name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    out = {"rows": rows, "members": "K = 1 by row", "calls": calls, "rounds": rounds, "library": "the experiments build, both sides",
           "order": "on, off, on, off, ...", "runs": runs}
    for kind in BOUNDED_KINDS:
        on, off = [r["p50_us"][kind] for r in runs["on"]], [r["p50_us"][kind] for r in runs["off"]]
        out[f"{kind}_p50_us"] = {"on": round(float(np.median(on)), 1), "off": round(float(np.median(off)), 1),
                                 "on_over_off": round(float(np.median(on)) / float(np.median(off)), 3),
                                 "off_spread": round((max(off) - min(off)) / float(np.median(off)), 3),
                                 "on_spread": round((max(on) - min(on)) / float(np.median(on)), 3)}
        assert [r["matches"][kind]["median_total"] for r in runs["on"]] == [r["matches"][kind]["median_total"] for r in runs["off"]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5, help="children per library")
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit")
    ap.add_argument("--shortcut-ab", action="store_true", help="the proven-in shortcut on and off (the experiments build)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--bounded", action="store_true", help="(child) the bounded kinds too: this tree's library only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.ab and not a.shortcut_ab:
        raise SystemExit("--ab LIB: the parent commit's library; or --shortcut-ab")
    text = json.dumps(run_shortcut(a.rows, a.calls, a.rounds) if a.shortcut_ab else run(a.ab, a.rows, a.calls, a.rounds), indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
