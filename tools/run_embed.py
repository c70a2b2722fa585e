"""EMBEDDING TABLES at 10 M rows, one handle, synchronous calls, top-100 (include/mi355rec_embed.h).
For d in --dims, both metrics and w_audio in {0, 1}:
    hybrid      EmbeddingTable.query with a fresh user vector per call: p50 per call of a pass of --calls calls, the median
                of --passes passes (the project's usual protocol);
    reads       the plain reads of the same buffers on the same box, device time per launch between two events around 20
                launches: the table (mi355rec_embed_enqueue_probe), and with w_audio != 0 the fp32 rows as well
                (mi355rec_enqueue_stream_probe) — the scores launch reads them — one after the other on one stream;
    host_blend  the only alternative without the table on the device: mi355rec_scores to the host, the similarity and the
                blend in numpy (a matrix-vector product, not the contract's tree), argpartition; --alt-calls calls.
Uniform random rows, a standard-normal table.

    python tools/run_embed.py --out profiles/r30_embed.json

--profile: few calls and no host_blend, for a run under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/run_embed.py --profile --dims 16
(one dim per run: the kernels of both dims share names only up to their template argument, the probes share theirs)."""
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


def reads_us(torch, eng, tab, with_rows, launches=20):
    """Device time per launch of the plain reads (events around `launches` of them on one stream)."""
    from spotify_recommender_amd import capi
    L = capi.lib()
    sink = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()

    def enqueue():
        tab.enqueue_probe(sink, stream)
        if with_rows:
            eng._check(L.mi355rec_enqueue_stream_probe(eng._h, sink.data_ptr(), stream.cuda_stream))

    with torch.cuda.stream(stream):
        for _ in range(3):
            enqueue()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(launches):
            enqueue()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def host_blend(eng, table, norms, user, audio_row, w_a, w_e, metric, topn):
    c = table @ user
    if metric == "cosine":
        c = c / (norms * np.linalg.norm(user))   # (the rows' norms are kept from one call to the next)
    v = w_e * c
    if w_a != 0.0:
        v = w_a * eng.scores_row(audio_row) + v
    top = np.argpartition(-v, topn)[:topn]
    return top[np.argsort(-v[top])]


def measure_dim(torch, a, d):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    n, topn = a.rows, 100
    rng = np.random.default_rng(30 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    norms = np.sqrt(np.einsum("ij,ij->i", table, table)) if not a.profile and a.alt_calls > 0 else None
    out = {}
    with CosineEngine(feats) as eng, EmbeddingTable(eng, table) as tab:
        info = tab.info()
        out["info"] = {k: info[k] for k in ("rows", "dim", "device_bytes", "tile_rows", "grid")}
        out["bytes_per_call"] = {"w_audio_0": n * 4 * d, "w_audio_1": n * (4 * d + 8 + 48)}
        for metric in ("cosine", "dot"):
            for w_a in (0.0, 1.0):
                kw = dict(metric=metric, embed_weight=0.05, audio_weight=w_a, topn=topn)
                call = lambda u: tab.query(user=u, audio_row=int(u[0] * 1e6) % n, **kw)
                for _ in range(5):
                    call(rng.standard_normal(d, dtype=F32))
                passes = [pass_p50_us(call, [rng.standard_normal(d, dtype=F32) for _ in range(a.calls)]) for _ in range(a.passes)]
                cell = {"hybrid_p50_us_median_of_passes": round(float(np.median(passes)), 1), "hybrid_p50_us_min": round(min(passes), 1),
                        "hybrid_p50_us_max": round(max(passes), 1), "reads_us_per_launch": round(reads_us(torch, eng, tab, w_a != 0.0), 1)}
                if not a.profile and a.alt_calls > 0:
                    users = [rng.standard_normal(d, dtype=F32) for _ in range(a.alt_calls)]
                    alt = lambda u: host_blend(eng, table, norms, u, 12345 % n, w_a, 0.05, metric, topn)
                    alt(users[0])
                    cell["host_blend_p50_us"] = round(pass_p50_us(alt, users), 1)
                out[f"{metric}_w_audio_{int(w_a)}"] = cell
                print(f"d = {d} {metric} w_audio = {w_a}: {cell}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--alt-calls", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.profile:
        a.calls, a.passes = 20, 1
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    doc = {"rows": a.rows, "topn": 100, "device": torch.cuda.get_device_name(0), "passes": a.passes, "calls_per_pass": a.calls,
           "protocol": "p50 per synchronous call, median of the passes; reads: device time per launch between two events"}
    for d in a.dims:
        doc[f"d{d}"] = measure_dim(torch, a, d)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
