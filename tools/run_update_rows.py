"""ROW UPDATES at 10 M x 12 on one handle with the replicas (include/mi355rec_diag.h, ROW UPDATES).  Three measurements, each
number the median of at least five runs that alternate within one process, timed with a host clock around the synchronous calls:

    cost       mi355rec_update_rows of 1, 1 000, 100 000 and 1 000 000 random rows; beside it mi355rec_rebuild_replica on the same
               handle, and destroying the handle and creating it again from host memory (labels set again where it had them).
               Without and with labels set.  CONDITION: 1 000 rows cost less than mi355rec_rebuild_replica in the same run.
    staleness  streamed single queries by row, top-100: us per query and rows sent to the exact chain per query (replica_counters)
               with everything fresh, after 1 % and after 10 % of the rows were updated with the bucketed sample and the anchor
               table left stale, and again after mi355rec_rebuild_replica.
    --ab DIR   `python bench.py --gpus 1 --steps 20 --warmup 5` three times per tree, alternating, this tree against a checkout of the
               parent commit built in DIR: the new tree's headline has to lie within the parent's own min-max spread (or above it).

    python tools/run_update_rows.py --out profiles/r18_update_rows.json --ab path/to/parent --ab-out profiles/r18_update_rows_ab.json"""
import argparse
import ctypes
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def figures(ts):
    a = np.asarray(ts)
    return {"median_ms": round(float(np.median(a)), 3), "min_ms": round(float(a.min()), 3), "max_ms": round(float(a.max()), 3), "runs": int(a.size)}


def cost(feats, labels, runs, sizes):
    from spotify_recommender_amd import CosineEngine, capi
    n = feats.shape[0]
    rng = np.random.default_rng(3)

    def create():
        eng = CosineEngine(feats)
        eng.set_replica(capi.REPLICA_ON)
        if labels is not None:
            eng.set_labels(labels)
        return eng

    eng = create()
    lists = {m: [(np.ascontiguousarray(rng.choice(n, size=m, replace=False).astype(np.int64)), rng.random((m, 12), dtype=np.float32))
                 for _ in range(runs + 1)] for m in sizes}
    times = {f"update_{m}": [] for m in sizes}
    times["rebuild_replica"], times["destroy_and_create"] = [], []

    def update(rows, new):
        capi.check(eng._lib.mi355rec_update_rows(eng._h, rows.ctypes.data_as(ctypes.c_void_p), rows.size, new.ctypes.data_as(ctypes.c_void_p)), eng._h)

    for m in sizes:                      # warm: the staging buffers, the label positions
        update(*lists[m][runs])
    for r in range(runs):                # the kinds alternate run by run
        for m in sizes:
            rows, new = lists[m][r]
            times[f"update_{m}"].append(ms(lambda: update(rows, new)))
        times["rebuild_replica"].append(ms(eng.rebuild_replica))

        def again():
            nonlocal eng
            eng.close()
            eng = create()
        times["destroy_and_create"].append(ms(again))
        for m in sizes:
            update(*lists[m][runs])      # (the fresh handle's staging, outside the timed calls)
    info = eng.update_info()
    eng.close()
    out = {k: figures(v) for k, v in times.items()}
    print("cost:", "with labels" if labels is not None else "without labels", out, file=sys.stderr, flush=True)
    out["update_1000_below_rebuild"] = bool(out["update_1000"]["median_ms"] < out["rebuild_replica"]["median_ms"])
    out["last_update_info"] = info
    return out


def staleness(feats, runs, queries, topn):
    import torch
    from spotify_recommender_amd import CosineEngine, capi
    n = feats.shape[0]
    rng = np.random.default_rng(5)
    qrows = rng.integers(0, n, size=queries)
    out = {}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        outs = torch.zeros((queries, topn), dtype=torch.int64, device="cuda:0")
        s = eng.own_stream()
        call = eng.bound_enqueue_row_keys_streamed(topn, stream=s)
        ptrs = [ctypes.c_void_p(outs[i].data_ptr()) for i in range(queries)]

        def stream():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r, p in zip(qrows, ptrs):
                call(int(r), p)
            eng.enqueue_flush(stream=s)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / queries * 1e6

        def state(name):
            stream()
            before = eng.replica_counters()
            ts = [stream() for _ in range(runs)]
            after = eng.replica_counters()
            out[name] = {"us_per_query_median": round(float(np.median(ts)), 2), "us_per_query_min": round(float(np.min(ts)), 2),
                         "us_per_query_max": round(float(np.max(ts)), 2), "runs": runs, "queries_per_run": queries,
                         "rescored_rows_per_query": (after["rescored_rows"] - before["rescored_rows"]) // (runs * queries),
                         "sample_last_used": eng.bucket_sample_info()["last_used"], "rows_since_snapshot": eng.update_info()["rows_since_snapshot"]}
            print("staleness:", name, out[name], file=sys.stderr, flush=True)

        state("fresh")
        done = np.zeros(n, dtype=bool)
        for name, frac in (("stale_1pct", 0.01), ("stale_10pct", 0.10)):
            want = int(n * frac) - int(done.sum())
            rows = rng.choice(np.flatnonzero(~done), size=want, replace=False).astype(np.int64)
            done[rows] = True
            eng.update_rows(rows, rng.random((rows.size, 12), dtype=np.float32))
            state(name)
        eng.rebuild_replica()
        state("after_rebuild")
    return out


def bench_value(tree, steps, warmup):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=str(tree),
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    return json.loads(line)


def ab(parent, rounds, steps=20, warmup=5):
    vals = {"parent": [], "new": []}
    metric = None
    for _ in range(rounds):              # alternating, the parent first
        for name, tree in (("parent", Path(parent).resolve()), ("new", ROOT)):
            doc = bench_value(tree, steps, warmup)
            print(f"bench {name}: {doc['value']}", file=sys.stderr, flush=True)
            metric = doc.get("metric", metric)
            vals[name].append(doc["value"])
    lo, hi = min(vals["parent"]), max(vals["parent"])
    new = float(np.median(vals["new"]))
    return {"command": f"python bench.py --gpus 1 --steps {steps} --warmup {warmup}", "metric": metric, "unit": "queries/s", "parent": vals["parent"],
            "new": vals["new"], "parent_min": lo, "parent_max": hi, "new_median": new, "new_within_parent_spread_or_above": bool(new >= lo)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5, help="runs per figure (at least 5)")
    ap.add_argument("--queries", type=int, default=1000, help="streamed queries per staleness run")
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", default="", help="a checkout of the parent commit, built")
    ap.add_argument("--ab-out", default="")
    ap.add_argument("--ab-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-steps", type=int, default=20, help="--ab: bench.py --steps (a longer timed region for a second opinion)")
    ap.add_argument("--ab-warmup", type=int, default=5)
    a = ap.parse_args()
    if a.runs < 5:
        raise SystemExit("--runs: at least 5")
    failed = []
    if not a.ab_only:
        import torch
        n = a.rows
        feats = np.random.default_rng(7).random((n, 12), dtype=np.float32)
        labels = np.random.default_rng(8).integers(0, 64, size=n).astype(np.int32)
        sizes = [m for m in (1, 1000, 100_000, 1_000_000) if m <= n]
        doc = {"rows": n, "device": torch.cuda.get_device_name(0), "clock": "host wall time around the synchronous calls",
               "cost_without_labels": cost(feats, None, a.runs, sizes), "cost_with_labels": cost(feats, labels, a.runs, sizes),
               "staleness_top%d_streamed" % a.topn: staleness(feats, a.runs, a.queries, a.topn)}
        failed += [f"{k}: 1 000 rows did not cost less than mi355rec_rebuild_replica" for k in ("cost_without_labels", "cost_with_labels")
                   if not doc[k]["update_1000_below_rebuild"]]
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(text + "\n")
    if a.ab:
        res = ab(a.ab, a.rounds, a.ab_steps, a.ab_warmup)
        if not res["new_within_parent_spread_or_above"]:
            failed.append("the new tree's headline is below the parent's own spread")
        text = json.dumps(res, indent=1)
        print(text)
        if a.ab_out:
            Path(a.ab_out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.ab_out).write_text(text + "\n")
    if failed:                           # the two conditions are gates: the figures are written, the run fails
        raise SystemExit("; ".join(failed))


if __name__ == "__main__":
    main()
