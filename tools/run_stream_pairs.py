"""Pairs and groups of streamed queries (mi355rec_set_stream_pairing), OFF against ON against GROUPS in ONE process: us per
query and rows sent to the exact chain per query for a stream of single queries dealt over the lanes as bench.py deals it
(four ring buffers per lane, the flush inside the timed region), over uniform catalogues of several sizes.  One JSON line per
row count — what the constants MI355REC_PAIRING_AUTO_MIN_ROWS (the smallest size at which neither topn is slower with pairs)
and MI355REC_GROUPS_AUTO_MIN_ROWS (the same for groups against pairs) are read from.

    python tools/run_stream_pairs.py [--rows 2500000,4000000,6000000,10000000] [--steps 300] [--rounds 3] [--lanes 2] > sweep.jsonl
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2500000,4000000,6000000,10000000")
    ap.add_argument("--topn", default="100,10")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=2, choices=[1, 2])
    args = ap.parse_args()
    import torch
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import CosineEngine, set_stream_pairing

    for n in (int(x) for x in args.rows.split(",")):
        f = torch.rand((n, 12), generator=torch.Generator(device="cuda").manual_seed(12345), device="cuda", dtype=torch.float32)
        line = {"rows": n, "steps": args.steps, "lanes": args.lanes}
        with CosineEngine(f) as eng:
            lanes = [eng, eng.lane()][:args.lanes]
            streams = [ln.own_stream() for ln in lanes]
            q_rows = [(k * 104729) % n for k in range(args.steps + args.warmup)]
            for topn in (int(x) for x in args.topn.split(",")):
                rings = [[torch.zeros(topn, dtype=torch.int64, device="cuda") for _ in range(4)] for _ in lanes]
                ptrs = [[ctypes.c_void_p(t.data_ptr()) for t in rs] for rs in rings]
                calls = [ln.bound_enqueue_row_keys_streamed(topn, s) for ln, s in zip(lanes, streams)]
                torch.cuda.synchronize()

                def region(lo, hi):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(lo, hi):
                        calls[k % args.lanes](q_rows[k], ptrs[k % args.lanes][(k // args.lanes) % 4])
                    for ln, s in zip(lanes, streams):
                        ln.enqueue_flush(stream=s)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0

                keys = {}
                modes = (("off", capi.PAIRING_OFF), ("on", capi.PAIRING_ON), ("groups", capi.PAIRING_GROUPS))
                for name, mode in modes:
                    line[f"top{topn}_{name}_us"] = []
                for _ in range(args.rounds):   # (alternating: a drift of the machine hits both alike)
                    for name, mode in modes:
                        for ln in lanes:
                            set_stream_pairing(ln, mode)
                        region(0, args.warmup)
                        before = sum(ln.replica_counters()["rescored_rows"] for ln in lanes)
                        pairs0 = sum(ln.stats().stream_pair_launches for ln in lanes)
                        groups0 = sum(ln.stats().stream_group_launches for ln in lanes)
                        dt = region(args.warmup, args.warmup + args.steps)
                        after = sum(ln.replica_counters()["rescored_rows"] for ln in lanes)
                        line[f"top{topn}_{name}_us"].append(round(dt / args.steps * 1e6, 2))
                        line[f"top{topn}_{name}_rescored"] = round((after - before) / args.steps)
                        line[f"top{topn}_{name}_pair_launches"] = sum(ln.stats().stream_pair_launches for ln in lanes) - pairs0
                        line[f"top{topn}_{name}_group_launches"] = sum(ln.stats().stream_group_launches for ln in lanes) - groups0
                        keys[name] = [[b.clone() for b in ring] for ring in rings]
                line[f"top{topn}_same_keys"] = all(torch.equal(a, b) for other in ("on", "groups")
                                                      for ra, rb in zip(keys["off"], keys[other]) for a, b in zip(ra, rb))
            for ln in lanes[1:]:
                ln.close()
        print(json.dumps(line), flush=True)
        del f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
