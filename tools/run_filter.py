"""Feature-filtered playlist queries at 10 M x 12, top-100, one handle, synchronous calls: p50 / p99 of
mi355rec_query_playlist_topn_where for K = 1 and 10 with one constrained feature passing about 90 %, 10 % and 1 % of the
rows of a uniform catalogue, beside, in the same process, the by-value single query, the unfiltered K = 1 / K = 10 playlist
calls and the fp32 route's single query (set_replica(OFF), measured last); the rows read from the fp32 matrix per query
(mi355rec_playlist_counters) and the kernel time of playlist_scan_kernel (HIP events: mi355rec_set_timing).
--ab LIB: also the unfiltered K = 1 / K = 10 calls with this build and with LIB (an earlier build), in child processes
alternating B, A, B, A ... (--rounds each), the two builds on the same box in one run.  Prints one JSON document and writes
it to --out.

    python tools/run_filter.py --out profiles/r08_filter.json [--ab path/to/parent/libmi355rec.so]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_filter -o filter -- python tools/run_filter.py --profile
(--profile: fewer calls, no A/B.)"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

RATES = {"pass_90pct": (0.05, 0.95), "pass_10pct": (0.45, 0.55), "pass_1pct": (0.495, 0.505)}
FEATURE = 2   # key: one constrained feature of a uniform catalogue, so the pass rate is known from the data


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


def catalogue(n):
    import torch
    return torch.rand((n, 12), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(7))


def ab(a):
    """The plain request, K = 1 and 10, on this tree and with the library a.ab in alternating child processes (tools/playlist_ab.py)."""
    from tools.playlist_ab import PLAIN, run
    return run(a.ab, a.rows, a.calls, a.topn, a.rounds, PLAIN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--ab", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from spotify_recommender_amd import CosineEngine, capi

    n, topn = a.rows, a.topn
    calls = 60 if a.profile else a.calls
    rng = np.random.default_rng(7)
    out = {"rows": n, "topn": topn, "device": torch.cuda.get_device_name(0), "feature": FEATURE, "cases": {}}
    data = catalogue(n)
    host_col = data[:, FEATURE].cpu().numpy()
    res = out["cases"]
    with CosineEngine(data) as eng:
        vecs = [data[int(r)].cpu().numpy() for r in rng.integers(0, n, size=calls)]
        res["by_value"] = timed(lambda q: eng.query_topn(q, -1, topn), vecs)
        for k in (1, 10):
            lists = [rng.choice(n, size=k, replace=False) for _ in range(calls)]
            cases = [(f"unfiltered_k{k}", None)] + [(f"{r}_k{k}", {FEATURE: b}) for r, b in RATES.items()]
            for key, where in cases:
                if a.profile and key != f"pass_10pct_k{k}" and key != f"unfiltered_k{k}":
                    continue
                call = lambda rows: eng.query_playlist_topn(rows, topn, where=where)   # noqa: E731
                res[key] = timed(call, lists)
                before = eng.playlist_counters()
                res[key]["playlist_scan_kernel_us"] = kernel_us(eng, call, lists[:100])
                after = eng.playlist_counters()
                res[key]["rows_exact_per_query"] = (after["rows_exact"] - before["rows_exact"]) // 100
                if where is not None:
                    lo, hi = where[FEATURE]
                    res[key]["pass_rate"] = round(float(((host_col >= lo) & (host_col <= hi)).mean()), 5)
        eng.set_replica(capi.REPLICA_OFF)   # (last: playlist calls of this handle would lose the 8-bit pre-filter too)
        res["by_value_fp32"] = timed(lambda q: eng.query_topn(q, -1, topn), vecs)
    del data
    torch.cuda.empty_cache()
    if not a.profile:
        for k in (1, 10):
            base = res[f"unfiltered_k{k}"]["p50_us"]
            for r in RATES:
                res[f"{r}_k{k}"]["ratio_to_unfiltered_p50"] = round(res[f"{r}_k{k}"]["p50_us"] / base, 3)
                res[f"{r}_k{k}"]["ratio_to_fp32_single_p50"] = round(res[f"{r}_k{k}"]["p50_us"] / res["by_value_fp32"]["p50_us"], 3)
        out["bars"] = {f"pass_90pct_k{k}_le_1.15x_unfiltered": res[f"pass_90pct_k{k}"]["ratio_to_unfiltered_p50"] <= 1.15 for k in (1, 10)}
        out["bars"].update({f"pass_1pct_k{k}_le_1.5x_fp32_single": res[f"pass_1pct_k{k}"]["ratio_to_fp32_single_p50"] <= 1.5
                            for k in (1, 10)})
        if a.ab:
            out["ab_unfiltered_vs_parent"] = ab(a)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
