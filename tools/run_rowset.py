"""ROW SETS at 10 M x 12, top-100, one handle with the 8-bit replica, synchronous calls (include/mi355rec_diag.h, ROW SETS; DESIGN.md
5.4.13).  In one process, on one handle over uniform random rows, members by row, for K = 1 and K = 10 and both metrics, the kinds
    no_set, no_set_again         the request without a set, twice: the second is the run's own spread
    exclude_empty                EXCLUDE with an empty set THROUGH THE KERNEL'S BRANCH: the pure cost of streaming the bits and of the
                                 load that is not prefetched.  (The library launches an empty EXCLUDE set as the plain request, so this
                                 kind uses a set of ONE row that no query can return: a member row of every request.)
    exclude_20k_random           EXCLUDE, 20 000 random ids
    exclude_20k_nearest          EXCLUDE, the query's own 20 000 nearest rows (one fixed query per K and metric: a history that sits
                                 where the taste is), beside no_set_fixed, the same query without the set
    only_50pct, only_1pct        ONLY, a random half / hundredth of the rows
alternate pass by pass (a pass = --calls synchronous calls, each ending in the host's wait for the result; its p50 is kept).  Per kind:
the median, minimum and maximum of the passes' p50 and the rows whose chains were computed per query (mi355rec_playlist_counters).
The yardstick for a set's own cost is no_set of the same run times (1 + 0.125 / 12) (the bytes streamed) plus the spread that
no_set_again shows.

--ab PARENT_LIB: calls WITHOUT a set must not slow down: tools/playlist_ab.py's run() over all of its kinds, this tree's library
against the parent commit's in alternating child processes; each ratio is read against the parent's own spread as that tool
reports it.  Written to --ab-out.

    python tools/run_rowset.py --out profiles/r17_rowset.json --ab path/to/parent/libmi355rec.so --ab-out profiles/r17_rowset_ab.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tools import playlist_ab  # noqa: E402


def nearest_rows(feats, rows, metric, count):
    """The `count` rows the request for `rows` ranks first (host arithmetic in float32: a choice of rows, not a result)."""
    q = feats[rows]
    if metric == "distance":
        v = np.zeros(feats.shape[0], np.float32)
        for m in range(q.shape[0]):
            v -= ((feats - q[m]) ** 2).sum(axis=1)
    else:
        norms = np.sqrt((feats * feats).sum(axis=1))
        v = np.zeros(feats.shape[0], np.float32)
        for m in range(q.shape[0]):
            v += (feats @ q[m]) / (norms * np.sqrt((q[m] * q[m]).sum()))
    return np.argpartition(-v, count)[:count].astype(np.int64)


def pass_p50_us(fn, args):
    import time
    ts = []
    for x in args:
        t0 = time.perf_counter()
        fn(x)
        ts.append(time.perf_counter() - t0)
    return float(np.percentile(np.asarray(ts) * 1e6, 50))


def measure(eng, cases, passes, calls):
    """{name: figures}; cases = {name: (fn, member lists)}: the cases alternate pass by pass."""
    for fn, lists in cases.values():
        for x in lists[:10]:
            fn(x)
    times = {name: [] for name in cases}
    for r in range(passes):
        for name, (fn, lists) in cases.items():
            times[name].append(pass_p50_us(fn, lists[r * calls:(r + 1) * calls]))
    out = {}
    for name, (fn, lists) in cases.items():
        ts = np.asarray(times[name])
        before = eng.playlist_counters()
        for x in lists[:20]:
            fn(x)
        after = eng.playlist_counters()
        out[name] = {"p50_us_median_of_passes": round(float(np.median(ts)), 1), "p50_us_min": round(float(ts.min()), 1),
                     "p50_us_max": round(float(ts.max()), 1), "passes": passes, "calls_per_pass": calls,
                     "rows_exact_per_query": (after["rows_exact"] - before["rows_exact"]) // 20}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=100, help="calls per pass")
    ap.add_argument("--passes", type=int, default=7, help="passes per kind (at least 5)")
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--history", type=int, default=20_000, help="ids of the two EXCLUDE kinds")
    ap.add_argument("--rounds", type=int, default=3, help="--ab: children per library")
    ap.add_argument("--ab-calls", type=int, default=300)
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit")
    ap.add_argument("--ab-out", default="")
    ap.add_argument("--ab-only", action="store_true", help="skip the kinds above")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.passes < 5:
        raise SystemExit("--passes: at least 5")
    if not a.ab_only:
        import torch
        from spotify_recommender_amd import CosineEngine, build, capi

        n, topn = a.rows, a.topn
        rng = np.random.default_rng(7)
        feats = rng.random((n, 12), dtype=np.float32)
        meta = [k for k in build.kernel_metadata() if "playlist_scan_kernel" in k["name"]][0]
        out = {"rows": n, "topn": topn, "device": torch.cuda.get_device_name(0), "history": a.history,
               "playlist_scan_kernel": {"vgpr": meta["vgpr"], "sgpr": meta["sgpr"], "lds": meta["lds"], "scratch": meta["scratch"]},
               "bytes_per_row": {"replica": 12, "set": 0.125}, "kinds": {}}
        with CosineEngine(feats) as eng:
            eng.set_replica(capi.REPLICA_ON)
            with eng.row_set(rng.choice(n, size=a.history, replace=False)) as random_ids, \
                    eng.row_set(np.flatnonzero(rng.random(n) < 0.5)) as half, eng.row_set(np.flatnonzero(rng.random(n) < 0.01)) as hundredth:
                for k in (1, 10):
                    # every request of this K holds row 0 as its first member: the one-row set {0} rejects nothing that could be returned
                    lists = [np.concatenate([[0], rng.choice(np.arange(1, n), size=k - 1, replace=False)]).astype(np.int64)
                             for _ in range(a.calls * a.passes)] if k > 1 else None
                    for metric in ("cosine", "distance"):
                        def call(rows, metric=metric, **kw):
                            if metric == "cosine":
                                return eng.query_playlist_topn(rows, topn, **kw)
                            return eng.query_nearest_rows_scaled(rows, topn, None, **kw)
                        if k == 1:
                            # K = 1: a one-row set per distinct member would be a set per call; the member is fixed instead
                            mine = [np.asarray([0], np.int64)] * (a.calls * a.passes)
                        else:
                            mine = lists
                        fixed = mine[0]
                        with eng.row_set([0]) as one_row, eng.row_set(nearest_rows(feats, fixed, metric, a.history)) as nearest:
                            cases = {
                                "no_set": (lambda rows, call=call: call(rows), mine),
                                "exclude_empty": (lambda rows, call=call, s=one_row: call(rows, seen=s), mine),
                                "exclude_20k_random": (lambda rows, call=call, s=random_ids: call(rows, seen=s), mine),
                                "only_50pct": (lambda rows, call=call, s=half: call(rows, only=s), mine),
                                "only_1pct": (lambda rows, call=call, s=hundredth: call(rows, only=s), mine),
                                "no_set_fixed": (lambda rows, call=call: call(rows), [fixed] * len(mine)),
                                "exclude_20k_nearest": (lambda rows, call=call, s=nearest: call(rows, seen=s), [fixed] * len(mine)),
                                "no_set_again": (lambda rows, call=call: call(rows), mine),
                            }
                            res = measure(eng, cases, a.passes, a.calls)
                        base = res["no_set"]["p50_us_median_of_passes"]
                        again = res["no_set_again"]["p50_us_median_of_passes"]
                        res["yardstick_us"] = round(base * (1 + 0.125 / 12) + abs(again - base), 1)
                        out["kinds"][f"{metric}_k{k}"] = res
        text = json.dumps(out, indent=1)
        print(text)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(text + "\n")
    if a.ab:
        doc = playlist_ab.run(a.ab, a.rows, a.ab_calls, a.topn, a.rounds, tuple(playlist_ab.kinds_of(None, 0)))
        for kind in playlist_ab.kinds_of(None, 0):
            row = doc[f"{kind}_p50_us"]
            row["within_parent_spread"] = bool(row["ratio"] <= 1.0 + row["parent_spread"])
        text = json.dumps(doc, indent=1)
        print(text)
        if a.ab_out:
            Path(a.ab_out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.ab_out).write_text(text + "\n")


if __name__ == "__main__":
    main()
