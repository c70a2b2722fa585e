#!/usr/bin/env python3
"""rocprofv3 --pmc counter_collection.csv files -> one small JSON under profiles/:
  python tools/summarize_pmc.py [--by-grid] profiles/r03_pmc_x.json "<command that was profiled>" <kernel substring> <dir> [<dir> ...]
Means per launch and launch counts per (kernel, counter); every directory is one --pmc pass of the same command.
--by-grid keeps launches of one kernel with different grids apart ("<kernel> [grid <threads>]": a pair launch and a launch for
two pairs are the same kernel).  Where the SQ counters are there, `derived` holds the shares read from them:
  waiting        SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES        of a wave's resident time, the part it waits for any instruction's result
  valu_of_wave   SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES     of a wave's resident time, the part a vector instruction of ITS is executing
                 (times the waves resident per SIMD: the SIMD's vector-active share)
  valu_active_per_busy_cycle   SQ_ACTIVE_INST_VALU / SQ_BUSY_CYCLES (the busy counter is per unit that reports it, not per SIMD)
  valu_insts     SQ_INSTS_VALU (wave instructions) per launch"""
import collections
import csv
import glob
import json
import os
import sys

argv = sys.argv[1:]
by_grid = argv[:1] == ["--by-grid"]
if by_grid:
    argv = argv[1:]
out_path, command, needle = argv[:3]
dirs = argv[3:]
kernels = collections.defaultdict(dict)
for d in dirs:
    f = max(glob.glob(f"{d}/**/*counter_collection.csv", recursive=True), key=os.path.getmtime)
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if needle in k:
            if by_grid:
                k = f"{k} [grid {r['Grid_Size']}]"
            agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k, cs in agg.items():
        for c, v in cs.items():
            kernels[k][c] = {"mean": sum(v) / len(v), "launches": len(v)}
derived = {}
for k, cs in kernels.items():
    m = {c: v["mean"] for c, v in cs.items()}
    if "SQ_WAVE_CYCLES" in m:
        x = {}
        if "SQ_WAIT_INST_ANY" in m:
            x["waiting"] = round(m["SQ_WAIT_INST_ANY"] / m["SQ_WAVE_CYCLES"], 4)
        if "SQ_ACTIVE_INST_VALU" in m:
            x["valu_of_wave"] = round(m["SQ_ACTIVE_INST_VALU"] / m["SQ_WAVE_CYCLES"], 4)
            if "SQ_BUSY_CYCLES" in m:
                x["valu_active_per_busy_cycle"] = round(m["SQ_ACTIVE_INST_VALU"] / m["SQ_BUSY_CYCLES"], 4)
        if "SQ_INSTS_VALU" in m:
            x["valu_insts"] = round(m["SQ_INSTS_VALU"])
        derived[k] = x
json.dump({"command": command,
           "units": "SQ_INSTS_* wave-instructions, SQ_*_CYCLES / SQ_WAIT_* quad-cycles summed over waves, GRBM_GUI_ACTIVE cycles "
                    "summed over the 8 XCDs, FETCH_SIZE / WRITE_SIZE KiB (FETCH_SIZE counts 64 B per 128-B request of a wide "
                    "coalesced read on gfx950: read bytes = 2 x FETCH_SIZE x 1024); means per launch",
           "kernels": kernels, **({"derived": derived} if derived else {})}, open(out_path, "w"), indent=1)
print(json.dumps({k: {c: round(v["mean"], 1) for c, v in cs.items()} for k, cs in kernels.items()}, indent=1))
if derived:
    print(json.dumps(derived, indent=1))
