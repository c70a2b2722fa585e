"""Label-filtered queries at 10 M x 12, 114 labels, topn 100, one handle: synchronous p50 / p99 of filtered queries for
label sets of 1, 8, 57 and 114 labels beside mi355rec_query_row_topn (unfiltered) on the same handle, the kernel time of
label_scan_kernel against scan_kernel's (HIP events on the dispatches: mi355rec_set_timing), and the wall time of
mi355rec_set_labels.  Two catalogues: uniform random rows with random labels, and genre-contiguous (labels in blocks, as a
preprocessed CSV is grouped).  Prints one JSON document and writes it to --out.

    python tools/run_labels.py --out profiles/r07_labels.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_labels -o labels -- python tools/run_labels.py --profile
(--profile: fewer queries, only the all-labels set and the unfiltered fp32 scan, so that the trace's per-kernel statistics
compare exactly those two.)"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def pct(ts, p):
    return float(np.percentile(np.asarray(ts) * 1e6, p))


def timed(fn, rows, warm=20):
    for r in rows[:warm]:
        fn(int(r))
    ts = []
    for r in rows:
        t0 = time.perf_counter()
        fn(int(r))
        ts.append(time.perf_counter() - t0)
    return {"p50_us": round(pct(ts, 50), 1), "p99_us": round(pct(ts, 99), 1), "queries": len(ts)}


def kernel_ms(eng, fn, rows):
    eng.set_timing(1)
    for r in rows:
        fn(int(r))
    ms = eng.stats().last_scan_ms
    eng.set_timing(0)
    return round(ms * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=400)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from spotify_recommender_amd import CosineEngine, capi

    n, topn = a.rows, a.topn
    nq = 60 if a.profile else a.queries
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    cats = {"uniform": rng.integers(0, 114, size=n).astype(np.int32),
            "genre_contiguous": (np.arange(n, dtype=np.int64) * 114 // n).astype(np.int32)}
    out = {"rows": n, "labels": 114, "topn": topn, "device": torch.cuda.get_device_name(0), "catalogues": {}}
    for cname, labels in cats.items():
        res = {}
        with CosineEngine(feats) as eng:
            t0 = time.perf_counter()
            eng.set_labels(labels)
            res["set_labels_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rows = rng.integers(0, n, size=nq)
            sizes = (114,) if a.profile else (1, 8, 57, 114)
            sets = {s: sorted(rng.choice(114, size=s, replace=False).tolist()) for s in sizes}
            if not a.profile:
                res["unfiltered_default_route"] = timed(lambda r: eng.query_row_topn(r, topn), rows)
            eng.set_replica(capi.REPLICA_OFF)   # single queries on the fp32 rows: scan_kernel, 48 B per row, as the filtered scan
            res["unfiltered_fp32"] = timed(lambda r: eng.query_row_topn(r, topn), rows)
            res["unfiltered_fp32"]["scan_kernel_us"] = kernel_ms(eng, lambda r: eng.query_row_topn(r, topn), rows[:100])
            for s, wanted in sets.items():
                key = f"labels_{s}"
                res[key] = timed(lambda r: eng.query_row_topn_labels(r, wanted, topn), rows)
                before = eng.label_counters()
                res[key]["label_scan_kernel_us"] = kernel_ms(eng, lambda r: eng.query_row_topn_labels(r, wanted, topn), rows[:100])
                after = eng.label_counters()
                res[key]["rows_scanned_per_query"] = (after["rows_scanned"] - before["rows_scanned"]) // 100
            eng.set_replica(capi.REPLICA_AUTO)
        res["bar_all_labels_kernel_ratio"] = round(res["labels_114"]["label_scan_kernel_us"] / res["unfiltered_fp32"]["scan_kernel_us"], 3)
        if "labels_1" in res:
            res["bar_one_label_p50_below_unfiltered"] = res["labels_1"]["p50_us"] < min(res["unfiltered_fp32"]["p50_us"],
                                                                                        res["unfiltered_default_route"]["p50_us"])
        out["catalogues"][cname] = res
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
