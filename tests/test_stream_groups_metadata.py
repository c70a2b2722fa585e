"""Two pairs per launch (scan_q8_kernel_pair's run-time `pairs` count) cost no kernel anything: the figures are read from the
gfx950 code objects inside the built library (no GPU needed: spotify_recommender_amd/build.py, kernel_metadata).

The library stays at sixty kernels — `pairs` is an argument, not an instantiation — with exactly one scan_q8_kernel_pair
inside the occupancy the launch geometry assumes (two workgroups of 512 threads per CU: <= 128 VGPRs, <= 80 KB of LDS, no
scratch: selecting the pair's arguments by a run-time index must not have moved the argument block to the stack).  Every OTHER
kernel's VGPR, LDS and scratch figures are those of the commit before (tests/golden/kernel_budgets_before_groups.json,
recorded with kernel_metadata from that commit's library)."""
import json
from pathlib import Path

import pytest

from spotify_recommender_amd import build

BEFORE = json.loads((Path(__file__).parent / "golden" / "kernel_budgets_before_groups.json").read_text())["kernels"]


@pytest.fixture(scope="module")
def kernels(engine_lib):
    return build.kernel_metadata(build.LIB_ENGINE)


def test_sixty_kernels(kernels):
    assert len(kernels) == 60, len(kernels)
    assert len(BEFORE) == 59


def test_one_pair_kernel_within_its_budgets(kernels):
    pair = [k for k in kernels if "scan_q8_kernel_pair" in k["name"]]
    assert len(pair) == 1, [k["name"] for k in pair]
    k = pair[0]
    assert k["vgpr"] <= 128 and k["lds"] <= 80 * 1024 and k["scratch"] == 0, k


def test_every_scan_q8_kernel_within_the_budgets(kernels):
    scans = [k for k in kernels if "scan_q8_kernel" in k["name"]]
    assert len(scans) == 6, [k["name"] for k in scans]
    for k in scans:
        assert k["vgpr"] <= 128 and k["lds"] <= 80 * 1024 and k["scratch"] == 0, k


def test_no_other_kernel_changed_in_any_figure(kernels):
    others = {k["name"]: [k["vgpr"], k["lds"], k["scratch"]] for k in kernels if "scan_q8_kernel_pair" not in k["name"]}
    assert sorted(others) == sorted(BEFORE), set(others) ^ set(BEFORE)
    changed = {n: (BEFORE[n], v) for n, v in others.items() if BEFORE[n] != v}
    assert not changed, changed
