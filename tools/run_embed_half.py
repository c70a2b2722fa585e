"""HALF-PRECISION EMBEDDING TABLES at 10 M rows, one handle, synchronous calls, top-100 (include/mi355rec_embed_half.h;
DESIGN.md 5.4.23).  For d in --dims, both storages, both metrics and w_audio in {0, 1}, in ONE run on one box:
    half        HalfEmbeddingTable.query with a fresh user vector per call: p50 per call of a pass of --calls calls, the
                median of --passes passes (the project's usual protocol);
    fp32        the baseline: EmbeddingTable (libmi355rec_embed.so, not touched by the half library) over the WIDENED table,
                the same users, the same protocol — both answer the same bits;
    reads       the plain read of the half table's bytes (mi355rec_embed_half_enqueue_probe) and of the fp32 table's, device
                time per launch between two events around 20 launches; with w_audio != 0 the fp32 audio rows as well.
Uniform random audio rows, a standard-normal table rounded to storage.

    python tools/run_embed_half.py --out profiles/r32_embed_half.json

--profile: few calls, for a run under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/run_embed_half.py --profile --dims 16
(one dim per run: the probes of both tables share one kernel name)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from run_embed import pass_p50_us, reads_us  # noqa: E402

F32 = np.float32


def measure_table(torch, a, eng, tab, d, rng, n):
    """{metric_w_audio_k: cell} of one attached table (half or fp32: the same calls)."""
    out = {}
    for metric in ("cosine", "dot"):
        for w_a in (0.0, 1.0):
            kw = dict(metric=metric, embed_weight=0.05, audio_weight=w_a, topn=100)
            call = lambda u: tab.query(user=u, audio_row=int(abs(u[0]) * 1e6) % n, **kw)
            for _ in range(5):
                call(rng.standard_normal(d, dtype=F32))
            passes = [pass_p50_us(call, [rng.standard_normal(d, dtype=F32) for _ in range(a.calls)]) for _ in range(a.passes)]
            out[f"{metric}_w_audio_{int(w_a)}"] = {
                "p50_us_median_of_passes": round(float(np.median(passes)), 1), "p50_us_min": round(min(passes), 1),
                "p50_us_max": round(max(passes), 1), "reads_us_per_launch": round(reads_us(torch, eng, tab, w_a != 0.0), 1)}
    return out


def measure_dim(torch, a, d):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    n = a.rows
    rng = np.random.default_rng(32 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    out = {"bytes_per_call": {"half_w_audio_0": n * 2 * d, "half_w_audio_1": n * (2 * d + 8 + 48), "fp32_w_audio_0": n * 4 * d,
                              "fp32_w_audio_1": n * (4 * d + 8 + 48)}}
    with CosineEngine(feats) as eng:
        for storage in a.storages:
            with HalfEmbeddingTable(eng, table, storage=storage) as tab:
                info = tab.info()
                cells = measure_table(torch, a, eng, tab, d, rng, n)
                out[storage] = {"info": {k: info[k] for k in ("rows", "dim", "device_bytes", "tile_rows", "grid", "storage")}, **cells}
                print(f"d = {d} {storage}: {cells}", file=sys.stderr, flush=True)
                if a.fp32 and storage == a.storages[0]:   # (one baseline per dim: the fp32 scan's time does not depend on the values)
                    wide = tab.widened()
                    with EmbeddingTable(eng, wide) as full:
                        probe_u = rng.standard_normal(d, dtype=F32)
                        h, f = tab.query(user=probe_u, topn=100), full.query(user=probe_u, topn=100)
                        assert h[0].tolist() == f[0].tolist() and np.array_equal(h[1].view(np.uint32), f[1].view(np.uint32))
                        base = measure_table(torch, a, eng, full, d, rng, n)
                        out["fp32_on_widened_" + storage] = {"info": {k: full.info()[k] for k in ("rows", "dim", "device_bytes", "tile_rows", "grid")}, **base}
                        print(f"d = {d} fp32 on the widened {storage} table: {base}", file=sys.stderr, flush=True)
                    del wide
    base_key = "fp32_on_widened_" + a.storages[0]
    if base_key in out:
        out["ratios"] = {storage: {cell: {"half_call_over_fp32_call": round(out[storage][cell]["p50_us_median_of_passes"] /
                                                                           out[base_key][cell]["p50_us_median_of_passes"], 3),
                                          "half_reads_over_fp32_reads": round(out[storage][cell]["reads_us_per_launch"] /
                                                                             out[base_key][cell]["reads_us_per_launch"], 3)}
                                   for cell in out[base_key] if cell != "info"} for storage in a.storages}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--storages", nargs="+", default=["fp16", "bf16"])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-fp32", dest="fp32", action="store_false")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.profile:
        a.calls, a.passes = 20, 1
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    doc = {"rows": a.rows, "topn": 100, "device": torch.cuda.get_device_name(0), "passes": a.passes, "calls_per_pass": a.calls,
           "protocol": "p50 per synchronous call, median of the passes; reads: device time per launch between two events; "
                       "fp32: EmbeddingTable over the widened table in the same run"}
    for d in a.dims:
        doc[f"d{d}"] = measure_dim(torch, a, d)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
