"""USER BATCHES at 10 M rows, one handle, synchronous calls, top-100 (include/mi355rec_embed_batch.h).
For d in --dims, both metrics and B in --batches, fresh user vectors per call:
    batch       EmbeddingBatchTable.query_users with B users: p50 per call of a pass of --calls calls, the median of --passes
                passes, per call and per user — for the product library and, with --pass-users, for the variants whose passes
                take P users at every dim (build.build_embed_batch(pass_users=P); built on the way if they are missing);
    sequential  the baseline in the same run: B calls of EmbeddingTable.query (mi355rec_embed_query, w_audio = 0) one after
                the other, timed as one block, per user.
Within a pass of the protocol the baseline and every variant are measured one after the other, B by B, so that what shares
the box shares it with all of them.  A standard-normal table.

    python tools/run_embed_batch.py --pass-users 1 2 4 8 --out profiles/r31_embed_batch.json

--profile: few calls, the product library at B = 8 and the plain read of the same bytes (embed_probe_kernel), for a run under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/run_embed_batch.py --profile --dims 16
(one dim per run: the kernels of the dims share names only up to their template arguments)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

F32 = np.float32


def pass_p50_us(fn, args):
    ts = []
    for x in args:
        t0 = time.perf_counter()
        fn(x)
        ts.append(time.perf_counter() - t0)
    return float(np.percentile(np.asarray(ts) * 1e6, 50))


def measure_dim(torch, a, d):
    from spotify_recommender_amd import CosineEngine, build
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
    n, topn = a.rows, 100
    rng = np.random.default_rng(31 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    out = {}
    libs = {"product": None}
    for p in a.pass_users:
        path = build.PKG / f"libmi355rec_embed_batch_p{p}.so"
        libs[f"P{p}"] = path if path.exists() else build.build_embed_batch(pass_users=p)
    with CosineEngine(feats) as eng, EmbeddingTable(eng, table) as single:
        tabs = {name: EmbeddingBatchTable(eng, table, lib_path=path) for name, path in libs.items()}
        try:
            info = tabs["product"].info()
            out["info"] = {k: info[k] for k in ("rows", "dim", "device_bytes", "tile_rows", "grid", "pass_users")}
            out["bytes_per_pass"] = n * 4 * d
            if a.profile:
                sink = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
                for _ in range(a.calls):
                    tabs["product"].query_users(users=rng.standard_normal((8, d), dtype=F32), topn=topn, metric="cosine", embed_weight=1.0)
                    single.enqueue_probe(sink)
                    torch.cuda.synchronize()
                return out
            for metric in ("cosine", "dot"):
                kw = dict(metric=metric, embed_weight=1.0, topn=topn)
                for B in a.batches:
                    def sequential(us):
                        for u in us:
                            single.query(user=u, audio_weight=0.0, **kw)
                    fns = {"sequential": sequential}
                    for name, tab in tabs.items():
                        fns[name] = lambda us, tab=tab: tab.query_users(users=us, **kw)
                    fresh = lambda count: [rng.standard_normal((B, d), dtype=F32) for _ in range(count)]
                    for fn in fns.values():
                        for us in fresh(3):
                            fn(us)
                    passes = {name: [] for name in fns}
                    for _ in range(a.passes):
                        for name, fn in fns.items():
                            passes[name].append(pass_p50_us(fn, fresh(a.calls)))
                    cell = {}
                    for name, ps in passes.items():
                        med = float(np.median(ps))
                        cell[name] = {"p50_us_per_call_median_of_passes": round(med, 1), "p50_us_per_user": round(med / B, 1),
                                      "p50_us_per_call_min": round(min(ps), 1), "p50_us_per_call_max": round(max(ps), 1)}
                    out[f"{metric}_B{B}"] = cell
                    print(f"d = {d} {metric} B = {B}: " + ", ".join(f"{k} {v['p50_us_per_user']}" for k, v in cell.items()) + " us per user",
                          file=sys.stderr, flush=True)
        finally:
            for tab in tabs.values():
                tab.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8, 64])
    ap.add_argument("--pass-users", type=int, nargs="*", default=[], help="also measure the variants with P users per pass")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.profile:
        a.calls, a.passes, a.pass_users = 20, 1, []
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    doc = {"rows": a.rows, "topn": 100, "device": torch.cuda.get_device_name(0), "passes": a.passes, "calls_per_pass": a.calls,
           "protocol": "p50 per synchronous call, median of the passes; sequential: B single calls timed as one block; fresh users per call"}
    for d in a.dims:
        doc[f"d{d}"] = measure_dim(torch, a, d)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
