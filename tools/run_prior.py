"""Playlist requests with a ROW PRIOR at 10 M x 12, top-100, one handle, synchronous calls (include/mi355rec_diag.h, ROW PRIORS;
DESIGN.md 5.4.9).  In one process, per catalogue and K = 1, 10 and 32: the request without a prior (the baseline) and the
same request with uniform and skewed (rand^4) priors at beta = 0.25 and 1.  Per case: p50 / p99, the kernel time of the scan
(HIP events: mi355rec_set_timing), the rows whose K chains were computed per query (mi355rec_playlist_counters), and the
ratio of the p50 and of the kernel time to the baseline's (the bytes predict 16 / 12 = 1.33).  Two catalogues: uniform random
rows, and genre-contiguous rows (114 clusters in blocks of row order, as a preprocessed CSV is grouped).
Prints one JSON document and writes it to --out.

    python tools/run_prior.py --out profiles/r13_prior.json
    python tools/run_prior.py --ab <libmi355rec.so of the parent commit> --out profiles/r13_prior_ab.json
(--ab: the request WITHOUT a prior, K = 1 and 10, on this tree and with the parent's library in alternating child processes:
the path this change must not slow down.)"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

N_CLUSTERS = 114


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


def catalogues(n, rng, only_uniform=False):
    yield "uniform", rng.random((n, 12), dtype=np.float32)
    if only_uniform:
        return
    centres = rng.random((N_CLUSTERS, 12), dtype=np.float32)
    block = (np.arange(n, dtype=np.int64) * N_CLUSTERS // n).astype(np.int64)
    f = centres[block] + rng.normal(0.0, 0.08, size=(n, 12)).astype(np.float32)
    yield "genre_contiguous", np.ascontiguousarray(np.clip(f, 0.0, 1.0), dtype=np.float32)


def ab(a):
    """The plain request, K = 1 and 10, on this tree and with the library a.ab in alternating child processes (tools/playlist_ab.py)."""
    from tools.playlist_ab import PLAIN, run
    return run(a.ab, a.rows, a.calls, a.topn, a.rounds, PLAIN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.ab:
        out = ab(a)
    else:
        import torch
        from spotify_recommender_amd import CosineEngine

        n, topn = a.rows, a.topn
        rng = np.random.default_rng(7)
        priors = {"uniform": rng.random(n, dtype=np.float32), "skewed": (rng.random(n, dtype=np.float32) ** 4).astype(np.float32)}
        out = {"rows": n, "topn": topn, "device": torch.cuda.get_device_name(0), "predicted_bytes_ratio": round(16 / 12, 3),
               "catalogues": {}}
        for cname, feats in catalogues(n, rng):
            res = {}
            with CosineEngine(feats) as eng:
                for k in (1, 10, 32):
                    lists = [rng.choice(n, size=k, replace=False) for _ in range(a.calls)]
                    block = {}
                    cases = [("no_prior", None, None)] + [(f"{pk}_beta{b}", pk, b) for pk in priors for b in (0.25, 1.0)]
                    loaded = None
                    for name, pk, beta in cases:
                        if pk is not None and pk != loaded:
                            t0 = time.perf_counter()
                            eng.set_priors(priors[pk])
                            res.setdefault("set_priors_ms", round((time.perf_counter() - t0) * 1e3, 1))
                            loaded = pk
                        fn = lambda rows, b=beta: eng.query_playlist_topn(rows, topn, prior_weight=b)   # noqa: E731
                        r = timed(fn, lists)
                        before = eng.playlist_counters()
                        r["playlist_scan_kernel_us"] = kernel_us(eng, fn, lists[:100])
                        after = eng.playlist_counters()
                        r["rows_exact_per_query"] = (after["rows_exact"] - before["rows_exact"]) // min(100, len(lists))
                        if "no_prior" in block:
                            r["p50_ratio_to_no_prior"] = round(r["p50_us"] / block["no_prior"]["p50_us"], 3)
                            r["kernel_ratio_to_no_prior"] = round(r["playlist_scan_kernel_us"] / block["no_prior"]["playlist_scan_kernel_us"], 3)
                        block[name] = r
                    res[f"k{k}"] = block
            out["catalogues"][cname] = res
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
