"""Which HIP runtime calls does one call of each synchronous entry point make?  Evidence for changes to the host code around
the launches (csrc/engine_sync.hip.h): run once on a build of the parent commit and once on the tree, the two reduced
files must be equal.

    rocprofv3 --hip-runtime-trace -f csv -d OUT -- python tools/sync_call_trace.py run OUT/labels.json
    python tools/sync_call_trace.py reduce OUT reduced.json

`run` makes the calls on one handle of 4 100 rows, one of 1 200 000 rows (8-bit replica: the lone-query path) and two node
handles on device 0, every entry point twice (the first call of a kind may allocate).  Before each call it calls
mi355rec_device_count() three times: three hipGetDeviceCount in a row are the separator `reduce` splits the calling thread's
trace at (no entry point calls it outside create).  `reduce` writes {"<k> <label>": [HIP call names in order]}, without the
hipStreamQuery calls: a wait for the completion word asks the stream about once a millisecond, so their number is timing."""
import csv
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

LABELS = []


def run():
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    lib = capi.lib()

    def mark(label, fn):
        for _ in range(2):
            for _ in range(3):
                lib.mi355rec_device_count()
            LABELS.append(label)
            fn()

    rng = np.random.default_rng(1)
    for n in (4100, 1_200_000):
        feats = rng.random((n, 12), dtype=np.float32)
        labels = (np.arange(n) % 2).astype(np.int32)
        groups = (np.arange(n) % 7).astype(np.int32)
        priors = rng.random(n, dtype=np.float32)
        rows, q, w = [5, 77, n - 1], feats[3], [1.0, -0.5, 1.0]
        with CosineEngine(feats) as e:
            for topn in (10, 1024, 1500, 2049, 3000):
                mark(f"n={n} query_row_topn {topn}", lambda: e.query_row_topn(9, topn))
                mark(f"n={n} query_topn {topn}", lambda: e.query_topn(q, -1, topn))
            for topn in (10, 682, 683):
                mark(f"n={n} query_batch_topn 3x{topn}", lambda: e.query_batch_topn(feats[:3], [0, 1, 2], topn))
            mark(f"n={n} query_batch_topn 1x10", lambda: e.query_batch_topn(feats[:1], [0], 10))
            for name, setter, a, b in (("labels", e.set_labels, labels, labels[::-1].copy()), ("groups", e.set_groups, groups, groups[::-1].copy()),
                                       ("priors", e.set_priors, priors, priors[::-1].copy())):
                mark(f"n={n} set_{name}", lambda: setter(a))
                mark(f"n={n} set_{name} again", lambda: setter(b))
                mark(f"n={n} set_{name} drop, then set", lambda: (setter(None), setter(a)))
            for topn in (10, 1024, 2049, 3000):
                mark(f"n={n} query_row_topn_labels {topn}", lambda: e.query_row_topn_labels(9, [0], topn))
                mark(f"n={n} query_topn_labels {topn}", lambda: e.query_topn_labels(q, -1, [0], topn))
            mark(f"n={n} labels nothing selected", lambda: e.query_row_topn_labels(9, [5], 10))
            for topn in (10, 1024):
                mark(f"n={n} query_playlist_topn {topn}", lambda: e.query_playlist_topn(rows, topn))
                mark(f"n={n} query_mean_topn {topn}", lambda: e.query_mean_topn(feats[rows], topn, exclude=[4]))
                mark(f"n={n} weighted where {topn}", lambda: e.query_playlist_topn(rows, topn, where={0: (0.1, 0.9)}, weights=w))
                mark(f"n={n} request labels prior {topn}", lambda: e.query_playlist_topn(rows, topn, labels=[1], prior_weight=0.5))
                mark(f"n={n} diverse {topn}", lambda: e.query_playlist_topn_diverse(rows, topn, 0.7, 1024))
                mark(f"n={n} capped {topn}", lambda: e.query_mean_topn_capped(feats[rows], topn, 2, 0.7, 1024))
            mark(f"n={n} fetch_rows 1500", lambda: e.fetch_rows(np.arange(1500) % n))
            mark(f"n={n} lane: create, query, destroy", lambda: (lambda lane: (lane.query_row_topn(9, 10), lane.query_playlist_topn_capped(rows, 10, 2),
                                                                               lane.close()))(e.lane()))
    feats = rng.random((4100, 12), dtype=np.float32)
    groups = (np.arange(4100) % 7).astype(np.int32)
    for devices, placement, name in (([0, 0, 0], capi.PLACEMENT_SHARDED, "sharded {0,0,0}"), ([0, 0], capi.PLACEMENT_REPLICATED, "replicated {0,0}")):
        with NodeEngine(feats, devices=devices, placement=placement) as nd:
            mark(f"{name} set_groups", lambda: nd.set_groups(groups))
            mark(f"{name} set_labels", lambda: nd.set_labels(groups % 2))
            mark(f"{name} set_priors", lambda: nd.set_priors(feats[:, 0]))
            mark(f"{name} capped 10", lambda: nd.query_playlist_topn_capped([5, 77], 10, 2, 0.7, 256))
            mark(f"{name} labels 10", lambda: nd.query_row_topn_labels(9, [0], 10))
            mark(f"{name} prior 10", lambda: nd.query_playlist_topn([5, 77], 10, prior_weight=0.5))
    for _ in range(3):
        lib.mi355rec_device_count()
    Path(sys.argv[2]).write_text(json.dumps(LABELS))


def reduce(out_dir, dest):
    """Splits the busiest thread's HIP calls at every run of three hipGetDeviceCount and names the pieces from labels.json."""
    files = sorted(Path(out_dir).rglob("*hip_api_trace.csv"))
    assert files, f"no *hip_api_trace.csv under {out_dir}"
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    by_thread = {}
    for r in rows:
        by_thread.setdefault(r["Thread_Id"], []).append(r)
    calls = max(by_thread.values(), key=lambda v: sum(1 for r in v if r["Function"] == "hipGetDeviceCount"))
    calls.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Function"] for r in calls if r["Function"] != "hipStreamQuery"]
    pieces, cur, i = [], None, 0
    while i < len(names):
        if names[i:i + 3] == ["hipGetDeviceCount"] * 3:
            if cur is not None:
                pieces.append(cur)
            cur, i = [], i + 3
            continue
        if cur is not None:
            cur.append(names[i])
        i += 1
    labels = json.loads(Path(out_dir, "labels.json").read_text())
    assert len(pieces) == len(labels), (len(pieces), len(labels))
    Path(dest).write_text(json.dumps({f"{k} {lab}": p for k, (lab, p) in enumerate(zip(labels, pieces))}, indent=0) + "\n")
    print(f"{len(pieces)} calls, {sum(len(p) for p in pieces)} HIP calls -> {dest}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        reduce(sys.argv[2], sys.argv[3])
