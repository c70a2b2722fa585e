"""The playlist family's three scans (playlist_scan_kernel, anyof_scan_kernel, manhattan_scan_kernel) call the tile loop's shared
pieces as functions of csrc/playlist.hip.h where they used to write them out: that cost no kernel of the library anything.  The
figures are read from the gfx950 code objects inside the built library (no GPU needed: spotify_recommender_amd/build.py,
kernel_metadata).

Every kernel's VGPR, SGPR, LDS and scratch figures are those of the commit before
(tests/golden/kernel_budgets_before_scan_parts.json, recorded with kernel_metadata from that commit's library), and the library
holds exactly those sixty kernels."""
import json
from pathlib import Path

import pytest

from spotify_recommender_amd import build

BEFORE = json.loads((Path(__file__).parent / "golden" / "kernel_budgets_before_scan_parts.json").read_text())["kernels"]


@pytest.fixture(scope="module")
def kernels(engine_lib):
    return {k["name"]: [k["vgpr"], k["sgpr"], k["lds"], k["scratch"]] for k in build.kernel_metadata(build.LIB_ENGINE)}


def test_the_same_sixty_kernels(kernels):
    assert len(BEFORE) == 60
    assert sorted(kernels) == sorted(BEFORE), set(kernels) ^ set(BEFORE)


def test_no_kernel_changed_in_any_figure(kernels):
    changed = {n: (BEFORE[n], v) for n, v in kernels.items() if BEFORE.get(n) != v}
    assert not changed, changed
