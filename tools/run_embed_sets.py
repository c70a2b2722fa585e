"""RESTRICTED EMBEDDING REQUESTS at 10 M rows, one handle, synchronous calls, top-100, cosine, w_audio = 0
(include/mi355rec_embed_sets.h).  For d in --dims and storage in --storages, in ONE run on one box, one
leg after the other, each with a fresh user vector per call — p50 per call of a pass of --calls calls, the median of
--passes passes:
    a   the baseline: EmbeddingTable / HalfEmbeddingTable (libraries this one does not touch) on the same table
    b   RestrictedEmbeddingTable, no sets
    c   seen = 20 000 random ids
    d   only = a random half, and a random 1 %
    e   only = one contiguous 1/114 of the rows (a genre of a catalogue grouped by genre), three such runs, and an empty
        run's fixed cost stand-in: a run of ONE row (launch, merge, copy, synchronise, one tile)
    f   c and e together
tiles_scored / tiles_total of one call stand beside every restricted leg.

    python tools/run_embed_sets.py --out profiles/r34_embed_sets.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from run_embed import pass_p50_us  # noqa: E402

F32 = np.float32


def leg(a, d, rng, call, tab=None):
    for _ in range(5):
        call(rng.standard_normal(d, dtype=F32))
    out = {}
    if tab is not None:
        before = tab.info()
        call(rng.standard_normal(d, dtype=F32))
        after = tab.info()
        out = {"tiles_scored": after["tiles_scored"] - before["tiles_scored"], "tiles_total": after["tiles_total"] - before["tiles_total"]}
    passes = [pass_p50_us(call, [rng.standard_normal(d, dtype=F32) for _ in range(a.calls)]) for _ in range(a.passes)]
    return {"p50_us_median_of_passes": round(float(np.median(passes)), 1), "p50_us_min": round(min(passes), 1),
            "p50_us_max": round(max(passes), 1), **out}


def measure(a, d, storage):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    from spotify_recommender_amd.embed_sets import RestrictedEmbeddingTable
    n = a.rows
    rng = np.random.default_rng(34 + d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    kw = dict(metric="cosine", embed_weight=1.0, topn=100)
    half = None if storage == "f32" else storage
    out = {}
    with CosineEngine(feats) as eng:
        with (EmbeddingTable(eng, table) if half is None else HalfEmbeddingTable(eng, table, storage=half)) as base:
            out["a_baseline"] = leg(a, d, rng, lambda u: base.query(user=u, **kw))
            probe = rng.standard_normal(d, dtype=F32)
            want = base.query(user=probe, **kw)
        with RestrictedEmbeddingTable(eng, table, storage=half) as tab:
            got = tab.query(user=probe, **kw)
            assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            run = n // 114
            starts = [n // 3, n // 3 + 5 * run, n // 3 + 11 * run]
            runs = [np.arange(s, s + run, dtype=np.int64) for s in starts]
            sets = {
                "seen_20000": tab.rowset(rng.choice(n, 20_000, replace=False)),
                "half": tab.rowset_from_mask(rng.random(n) < 0.5),
                "percent": tab.rowset_from_mask(rng.random(n) < 0.01),
                "run": tab.rowset(runs[0]),
                "three_runs": tab.rowset(np.concatenate(runs)),
                "one_row": tab.rowset([n // 2]),
            }
            info = tab.info()
            out["info"] = {k: info[k] for k in ("rows", "dim", "device_bytes", "tile_rows", "grid", "storage")}
            legs = [("b_no_sets", dict()), ("c_seen_20000", dict(seen=sets["seen_20000"])), ("d_only_half", dict(only=sets["half"])),
                    ("d_only_percent", dict(only=sets["percent"])), ("e_only_run", dict(only=sets["run"])),
                    ("e_only_three_runs", dict(only=sets["three_runs"])), ("e_only_one_row", dict(only=sets["one_row"])),
                    ("f_run_and_seen", dict(only=sets["run"], seen=sets["seen_20000"]))]
            for name, sk in legs:
                out[name] = leg(a, d, rng, lambda u, sk=sk: tab.query(user=u, **kw, **sk), tab)
                print(f"d = {d} {storage} {name}: {out[name]}", file=sys.stderr, flush=True)
            for s in sets.values():
                s.close()
    base_us = out["a_baseline"]["p50_us_median_of_passes"]
    fixed = out["e_only_one_row"]["p50_us_median_of_passes"]
    out["ratios_to_a"] = {name: round(out[name]["p50_us_median_of_passes"] / base_us, 3) for name, _ in legs}
    out["e_model_us"] = {name: round(fixed + base_us * out[name]["tiles_scored"] / out[name]["tiles_total"], 1)
                         for name in ("e_only_run", "e_only_three_runs", "f_run_and_seen")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--storages", nargs="+", default=["f32", "fp16"])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    doc = {"rows": a.rows, "topn": 100, "metric": "cosine", "w_audio": 0, "device": torch.cuda.get_device_name(0), "passes": a.passes,
           "calls_per_pass": a.calls,
           "protocol": "p50 per synchronous call, median of the passes, a fresh user per call, all legs in one run; e_model_us: the "
                       "one-row leg (the call's fixed cost) + the baseline scaled by tiles_scored / tiles_total"}
    for d in a.dims:
        for storage in a.storages:
            doc[f"d{d}_{storage}"] = measure(a, d, storage)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
