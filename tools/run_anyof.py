"""ANY-OF REQUESTS at 10 M x 12, one handle with the 8-bit replica, synchronous calls, top-100 (include/mi355rec_diag.h, ANY-OF
REQUESTS).  In one process, on one handle, members by row, for K = 1, 3, 10, 32 the kinds
    anyof                  the any-of request without out_member (scan, merge; the merge notifies)
    anyof_member           the same with out_member (scan, merge, attribution launch, a copy back, a stream wait)
    k_one_member           what a caller must do today: K one-member playlist requests with the whole exclusion list, then the host
                           merge (max per row, canonical order, the first N)
    mean                   the mean playlist request with the same members
alternate pass by pass (a pass = --calls synchronous calls with fresh members; its p50 is kept).  Per kind: the median, minimum and
maximum of the passes' p50, and rows_exact per call (mi355rec_playlist_counters) of anyof and mean.  Two catalogues: uniform random
rows, and spotify_recommender_amd.synth.clustered_catalogue(300 clusters, spread 0.01, contiguous, genre ramp), where the starting
threshold matters.

    python tools/run_anyof.py --out profiles/r22_anyof.json

--ab LIB: the A/B against another build of the library (the parent commit's): tools/playlist_ab.py's plain_k1 and distance_k1 in
ALTERNATING child processes, --rounds children a side, and the create time (the fp16 self-check now rides in replica_build_kernel).

    python tools/run_anyof.py --ab path/to/parent/libmi355rec.so --out profiles/r22_anyof_ab.json"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from playlist_ab import run  # noqa: E402

KS = (1, 3, 10, 32)


def pass_p50_us(fn, args):
    ts = []
    for x in args:
        t0 = time.perf_counter()
        fn(x)
        ts.append(time.perf_counter() - t0)
    return float(np.percentile(np.asarray(ts) * 1e6, 50))


def host_merge(eng, rows, topn):
    best = {}
    excl = rows.tolist()
    for r in rows:
        ids, sc = eng.query_playlist_topn(np.asarray([r], np.int64), topn, exclude=excl)
        for i, s in zip(ids.tolist(), sc.tolist()):
            if i not in best or s > best[i]:
                best[i] = s
    order = sorted(best, key=lambda i: (-best[i], i))[:topn]
    return order


def measure_catalogue(eng, n, a, topn):
    import ctypes
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import query_anyof

    def anyof_plain(rows):   # no out_member: the raw call (engine.query_anyof always asks for it)
        idx = np.empty(topn, np.int64)
        sc = np.empty(topn, np.float32)
        c = ctypes.c_int(0)
        q = capi.AnyOfQuery()
        q.size = ctypes.sizeof(capi.AnyOfQuery)
        q.rows, q.k, q.topn = rows.ctypes.data_as(ctypes.c_void_p), rows.size, topn
        res = capi.AnyOfResult(idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), None, ctypes.pointer(c))
        capi.check(eng._lib.mi355rec_query_anyof_request(eng._h, ctypes.byref(q), None, ctypes.byref(res)), eng._h)

    rng = np.random.default_rng(22)
    out = {}
    for k in KS:
        kinds = {"anyof": anyof_plain, "anyof_member": lambda rows: query_anyof(eng, topn, rows=rows),
                 "k_one_member": lambda rows: host_merge(eng, rows, topn), "mean": lambda rows: eng.query_playlist_topn(rows, topn)}
        times = {name: [] for name in kinds}
        exact = {}
        for fn in kinds.values():
            for _ in range(3):
                fn(np.ascontiguousarray(rng.choice(n, size=k, replace=False).astype(np.int64)))
        for _ in range(a.passes):
            for name, fn in kinds.items():
                calls = a.calls if name != "k_one_member" else max(5, a.calls // k)
                lists = [np.ascontiguousarray(rng.choice(n, size=k, replace=False).astype(np.int64)) for _ in range(calls)]
                before = eng.playlist_counters()["rows_exact"]
                times[name].append(pass_p50_us(fn, lists))
                exact.setdefault(name, []).append((eng.playlist_counters()["rows_exact"] - before) / calls)
        out[f"k{k}"] = {name: {"p50_us_median_of_passes": round(float(np.median(ts)), 1), "p50_us_min": round(float(np.min(ts)), 1),
                               "p50_us_max": round(float(np.max(ts)), 1), "rows_exact_per_call": round(float(np.median(exact[name])), 1)}
                        for name, ts in times.items()}
        r = out[f"k{k}"]
        r["anyof_over_k_one_member"] = round(r["anyof"]["p50_us_median_of_passes"] / r["k_one_member"]["p50_us_median_of_passes"], 3)
        r["anyof_member_over_k_one_member"] = round(r["anyof_member"]["p50_us_median_of_passes"] / r["k_one_member"]["p50_us_median_of_passes"], 3)
        print(f"K = {k}: " + ", ".join(f"{name} {r[name]['p50_us_median_of_passes']} us" for name in kinds), file=sys.stderr, flush=True)
    return out


def main_measure(a):
    import torch
    from spotify_recommender_amd import CosineEngine, build, capi
    from spotify_recommender_amd.synth import clustered_catalogue

    n, topn = a.rows, 100
    meta = {f: [k for k in build.kernel_metadata() if f in k["name"]][0] for f in ("anyof_scan_kernel", "playlist_scan_kernel", "replica_build_kernel")}
    out = {"rows": n, "topn": topn, "members": "by row", "replica": "on", "device": torch.cuda.get_device_name(0), "passes": a.passes,
           "calls_per_pass": a.calls, "kernels": {f: {x: m[x] for x in ("vgpr", "sgpr", "lds", "scratch")} for f, m in meta.items()}}
    feats = np.random.default_rng(21).random((n, 12), dtype=np.float32)
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        out["uniform"] = measure_catalogue(eng, n, a, topn)
    del feats
    clusters = max(2, 300 * n // 10_000_000)
    t = clustered_catalogue(n, 0.01, clusters=clusters, contiguous=True, ramp=True, device="cuda:0")
    with CosineEngine(t) as eng:
        eng.set_replica(capi.REPLICA_ON)
        out["clustered_300_sorted"] = measure_catalogue(eng, n, a, topn)
    return out


def create_ms(lib, rows, rounds):
    """Median wall time of CosineEngine(feats) in child processes of each library, alternating (the folded kernel's route)."""
    import os
    import subprocess
    code = ("import sys,time,numpy as np;sys.path.insert(0,%r);from spotify_recommender_amd import CosineEngine;"
            "f=np.random.default_rng(7).random((%d,12),dtype=np.float32);e=CosineEngine(f);e.close();ts=[]\n"
            "for _ in range(5):\n t0=time.perf_counter();e=CosineEngine(f);ts.append(time.perf_counter()-t0);e.close()\n"
            "print('MS',round(1e3*sorted(ts)[2],2))") % (str(Path(__file__).resolve().parents[1]), rows)
    env_this = dict(os.environ)
    env_this.pop("MI355REC_LIB", None)
    env_parent = dict(os.environ, MI355REC_LIB=str(Path(lib).resolve()), MI355REC_CAPI_LENIENT="1")
    res = {"this": [], "parent": []}
    for _ in range(rounds):
        for name, env in (("this", env_this), ("parent", env_parent)):
            p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"create child ({name}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res[name].append(float([l for l in p.stdout.splitlines() if l.startswith("MS ")][-1][3:]))
    return {"runs": res, "this": float(np.median(res["this"])), "parent": float(np.median(res["parent"])),
            "parent_min": min(res["parent"]), "parent_max": max(res["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=60, help="calls per pass (A/B: per kind and child)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="A/B: children per library")
    ap.add_argument("--ab", default="", help="libmi355rec.so built from the parent commit: run the A/B instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.ab:
        doc = run(a.ab, a.rows, a.calls, 100, a.rounds, ("plain_k1", "distance_k1"))
        doc["create_ms"] = create_ms(a.ab, a.rows, a.rounds)
    else:
        doc = main_measure(a)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
