"""Playlist calls within a label set at 10 M x 12, 114 labels, top-100, one handle, synchronous calls (include/mi355rec_diag.h,
PLAYLIST REQUESTS).  In one process, per catalogue: the unlabelled playlist call at K = 1, 10 and 32 (the
baseline), the same calls with all 114 labels, 3 labels and 1 label selected, and at K = 1 mi355rec_query_row_topn_labels
for the same selections.  Per case: p50 / p99, the kernel time of the scan (HIP events: mi355rec_set_timing), for the
playlist calls the rows whose K chains were computed per query (mi355rec_playlist_counters), and the ratio of the p50 and of
the kernel time to the unlabelled call's (the bytes predict 14 / 12 = 1.17 for the all-labels case).  Two catalogues over
the same rows: uniform random labels, and genre-contiguous labels (blocks in row order, as a preprocessed CSV is grouped).
Prints one JSON document and writes it to --out.

    python tools/run_playlist_labels.py --out profiles/r12_playlist_labels.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_playlist_labels -o playlist_labels -- \\
        python tools/run_playlist_labels.py --profile
(--profile: fewer calls, the uniform catalogue, K = 10 with all labels selected and the label route with all labels, so that
the trace's per-kernel statistics are those of exactly these two kernels' labelled launches.)"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

N_LABELS = 114


def pct(ts, p):
    return float(np.percentile(np.asarray(ts) * 1e6, p))


def timed(fn, args, warm=20):
    for x in args[:warm]:
        fn(x)
    ts = []
    for x in args:
        t0 = time.perf_counter()
        fn(x)
        ts.append(time.perf_counter() - t0)
    return {"p50_us": round(pct(ts, 50), 1), "p99_us": round(pct(ts, 99), 1), "calls": len(ts)}


def kernel_us(eng, fn, args):
    eng.set_timing(1)
    for x in args:
        fn(x)
    ms = eng.stats().last_scan_ms
    eng.set_timing(0)
    return round(ms * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from spotify_recommender_amd import CosineEngine

    n, topn = a.rows, a.topn
    calls = 60 if a.profile else a.calls
    rng = np.random.default_rng(7)
    feats = rng.random((n, 12), dtype=np.float32)
    cats = {"uniform": rng.integers(0, N_LABELS, size=n).astype(np.int32),
            "genre_contiguous": (np.arange(n, dtype=np.int64) * N_LABELS // n).astype(np.int32)}
    if a.profile:
        cats = {"uniform": cats["uniform"]}
    three = sorted(rng.choice(N_LABELS, size=3, replace=False).tolist())
    selections = {"all_114": list(range(N_LABELS)), "labels_3": three, "labels_1": three[:1]}
    if a.profile:
        selections = {"all_114": selections["all_114"]}
    out = {"rows": n, "labels": N_LABELS, "topn": topn, "device": torch.cuda.get_device_name(0),
           "selections": selections, "predicted_all_labels_ratio": round(14 / 12, 3), "catalogues": {}}
    for cname, labels in cats.items():
        res = {}
        with CosineEngine(feats) as eng:
            t0 = time.perf_counter()
            eng.set_labels(labels)
            res["set_labels_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            res["selected_rows"] = {s: int(np.isin(labels, w).sum()) for s, w in selections.items()}
            for k in ((10,) if a.profile else (1, 10, 32)):
                lists = [rng.choice(n, size=k, replace=False) for _ in range(calls)]
                cases = {} if a.profile else {"unlabelled": None}
                cases.update(selections)
                block = {}
                for sname, wanted in cases.items():
                    fn = lambda rows, w=wanted: eng.query_playlist_topn(rows, topn, labels=w)   # noqa: E731
                    r = timed(fn, lists)
                    before = eng.playlist_counters()
                    r["playlist_scan_kernel_us"] = kernel_us(eng, fn, lists[:100])
                    after = eng.playlist_counters()
                    r["rows_exact_per_query"] = (after["rows_exact"] - before["rows_exact"]) // min(100, len(lists))
                    if "unlabelled" in block:
                        r["p50_ratio_to_unlabelled"] = round(r["p50_us"] / block["unlabelled"]["p50_us"], 3)
                        r["kernel_ratio_to_unlabelled"] = round(r["playlist_scan_kernel_us"] / block["unlabelled"]["playlist_scan_kernel_us"], 3)
                    block[sname] = r
                if k == 1 or a.profile:   # the label route's single query for the same selections
                    for sname, wanted in selections.items():
                        fn = lambda rows, w=wanted: eng.query_row_topn_labels(int(rows[0]), w, topn)   # noqa: E731
                        r = timed(fn, lists)
                        r["label_scan_kernel_us"] = kernel_us(eng, fn, lists[:100])
                        block["label_route_" + sname] = r
                res[f"k{k}"] = block
        out["catalogues"][cname] = res
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
