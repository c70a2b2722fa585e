"""Weighted playlist queries at 10 M x 12, top-100, one handle, synchronous calls: p50 / p99 of
mi355rec_query_playlist_topn_weighted, the rows read from the fp32 matrix per query (mi355rec_playlist_counters), the kernel
time of playlist_scan_kernel (HIP events: mi355rec_set_timing) and the median |u| of the weighted mean direction, on a
uniform catalogue and on the 3000-cluster one (contiguous clusters; likes from one cluster, dislikes from another):
  * K = 10, random positive weights in [0.25, 4], beside the unweighted call of the same members (bar: within 3 %);
  * 7 likes + 3 dislikes at -0.5 and at -1.0, beside the likes-only call of the same 7 songs (recorded, no bar).
--ab LIB: also the unweighted K = 1 / K = 10 calls with this build and with LIB (an earlier build), in child processes
alternating this, parent, this, parent ... (--rounds each) on the same box in one run (bar: ratio of the median p50s <= 1.03).
Prints one JSON document and writes it to --out.

    python tools/run_weighted.py --out profiles/r09_weighted.json [--ab path/to/parent/libmi355rec.so]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_weighted -o weighted -- python tools/run_weighted.py --profile
(--profile: fewer calls, the uniform catalogue only, no A/B.)"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tools.run_filter import catalogue, kernel_us, timed  # noqa: E402


def mean_norm(members, w):
    """|u| of u = (sum_k w_k q_k / |q_k|) / sum_k |w_k| (float64: a figure for the report, not the kernel's bits)."""
    m = np.asarray(members, np.float64)
    w = np.asarray(w, np.float64)
    u = (w[:, None] * m / np.linalg.norm(m, axis=1, keepdims=True)).sum(0) / np.abs(w).sum()
    return float(np.linalg.norm(u))


def ab(a):
    """The plain request, K = 1 and 10, on this tree and with the library a.ab in alternating child processes (tools/playlist_ab.py)."""
    from tools.playlist_ab import PLAIN, run
    return run(a.ab, a.rows, a.calls, a.topn, a.rounds, PLAIN)


def measure(eng, host, topn, lists, weights):
    """One case: lists[i] (rows) with weights[i] (None: the unweighted entry point)."""
    args = list(zip(lists, weights))
    call = lambda x: eng.query_playlist_topn(x[0], topn, weights=x[1])   # noqa: E731
    r = timed(call, args)
    probe = args[:100]
    before = eng.playlist_counters()
    r["playlist_scan_kernel_us"] = kernel_us(eng, call, probe)
    after = eng.playlist_counters()
    r["rows_exact_per_query"] = (after["rows_exact"] - before["rows_exact"]) // len(probe)
    r["median_mean_norm"] = round(float(np.median([mean_norm(host(rows), np.ones(len(rows)) if w is None else w) for rows, w in probe])), 4)
    return r


def cases_for(eng, host, topn, calls, likes_of, dislikes_of, rng, profile):
    res = {}
    ten = [np.concatenate([likes_of(i), dislikes_of(i)]) for i in range(calls)]
    seven = [rows[:7] for rows in ten]
    none = [None] * calls
    res["unweighted_k10"] = measure(eng, host, topn, ten, none)
    res["positive_k10"] = measure(eng, host, topn, ten, [rng.uniform(0.25, 4.0, 10).astype(np.float32) for _ in range(calls)])
    if profile:
        return res
    res["likes_only_k7"] = measure(eng, host, topn, seven, none)
    for name, dw in (("dislikes_0.5", 0.5), ("dislikes_1.0", 1.0)):
        w = np.array([1.0] * 7 + [-dw] * 3, np.float32)
        res[f"likes7_{name}"] = measure(eng, host, topn, ten, [w] * calls)
    base = res["unweighted_k10"]
    res["positive_k10"]["ratio_to_unweighted_p50"] = round(res["positive_k10"]["p50_us"] / base["p50_us"], 3)
    res["positive_k10"]["ratio_to_unweighted_rows_exact"] = round(res["positive_k10"]["rows_exact_per_query"] / max(base["rows_exact_per_query"], 1), 3)
    likes = res["likes_only_k7"]
    for name in ("dislikes_0.5", "dislikes_1.0"):
        r = res[f"likes7_{name}"]
        r["ratio_to_likes_only_p50"] = round(r["p50_us"] / likes["p50_us"], 3)
        r["ratio_to_likes_only_rows_exact"] = round(r["rows_exact_per_query"] / max(likes["rows_exact_per_query"], 1), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--clusters", type=int, default=3000)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--ab", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.synth import clustered_catalogue

    n, topn = a.rows, a.topn
    calls = 60 if a.profile else a.calls
    out = {"rows": n, "topn": topn, "calls": calls, "device": torch.cuda.get_device_name(0)}

    rng = np.random.default_rng(7)
    data = catalogue(n)
    host = lambda rows: data[torch.as_tensor(np.asarray(rows), device=data.device)].cpu().numpy()   # noqa: E731
    draws = [rng.choice(n, size=10, replace=False) for _ in range(calls)]
    with CosineEngine(data) as eng:
        out["uniform"] = cases_for(eng, host, topn, calls, lambda i: draws[i][:7], lambda i: draws[i][7:], rng, a.profile)
    del data
    torch.cuda.empty_cache()

    if not a.profile:
        data = clustered_catalogue(n, 0.03, seed=4242 + a.clusters, clusters=a.clusters, contiguous=True, ramp=False)
        per = n // a.clusters
        like_c = rng.integers(0, a.clusters, size=calls)
        dis_c = (like_c + rng.integers(1, a.clusters, size=calls)) % a.clusters     # another cluster
        inner = lambda c, k: c * per + per // 4 + rng.choice(per // 2, size=k, replace=False)   # noqa: E731  (inside the cluster's rows)
        likes = [inner(int(c), 7) for c in like_c]
        dislikes = [inner(int(c), 3) for c in dis_c]
        with CosineEngine(data) as eng:
            out["clustered"] = cases_for(eng, host, topn, calls, lambda i: likes[i], lambda i: dislikes[i], rng, False)
            out["clustered"]["note"] = ("unweighted_k10 / positive_k10: the 7 songs of one cluster and the 3 of another, all liked; "
                                        "likes7_dislikes_*: the 3 of the other cluster disliked")
        del data
        torch.cuda.empty_cache()
        out["bars"] = {f"{c}_positive_k10_le_1.03x_unweighted": out[c]["positive_k10"]["ratio_to_unweighted_p50"] <= 1.03
                       for c in ("uniform", "clustered")}
        out["rows_exact_more_than_doubles_with_dislikes"] = {
            f"{c}_{name}": out[c][f"likes7_{name}"]["ratio_to_likes_only_rows_exact"] > 2.0
            for c in ("uniform", "clustered") for name in ("dislikes_0.5", "dislikes_1.0")}
        if a.ab:
            out["ab_unweighted_vs_parent"] = ab(a)
            out["bars"]["unweighted_k1_k10_le_1.03x_parent"] = out["ab_unweighted_vs_parent"]["within_3pct"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
