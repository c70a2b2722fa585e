"""csrc/shard_merge.h — the host merge of a row-sharded node handle (merge_over_shards in csrc/node_state.hip.h) — where no GPU is:
pure arithmetic on packed uint64 keys, so a wrong tie order, a dropped total or a tag that does not follow its key shows here, in
a stand-alone program (tests/shard_merge_check.cpp) under AddressSanitizer and UBSan, run as its own process.  The GPU leg, which
runs the merge behind real shards, is tests/test_gpu_node_sweep.py."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


@pytest.fixture(scope="module")
def shard_merge_check(tmp_path_factory):
    """tests/shard_merge_check.cpp built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("shard_merge") / "shard_merge_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           str(ROOT / "tests" / "shard_merge_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_shard_merge_h_under_sanitizers(shard_merge_check):
    p = subprocess.run([str(shard_merge_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "shard_merge.h: ok" in p.stdout, p.stdout + p.stderr
