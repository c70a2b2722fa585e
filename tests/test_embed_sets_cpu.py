"""RESTRICTED EMBEDDING REQUESTS without a GPU (include/mi355rec_embed_sets.h): csrc/embed_sets_request.h — the bitmap
builder, the no-launch predicates and the ext's size rule — as a stand-alone program (tests/embed_sets_check.cpp) under
AddressSanitizer and UBSan, run as its own process; that the builder includes no HIP header; and what
RestrictedEmbeddingTable refuses before any native call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import embed_cases as ec

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


@pytest.fixture(scope="module")
def embed_sets_check(tmp_path_factory):
    """tests/embed_sets_check.cpp, built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed_sets") / "embed_sets_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_sets_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_sets_request_h_under_sanitizers(embed_sets_check):
    p = subprocess.run([str(embed_sets_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_sets_request.h: ok" in p.stdout, p.stdout + p.stderr


def test_the_builder_is_host_only():
    """embed_sets_request.h and what it includes from csrc name no HIP header (g++ compiled it above)."""
    seen, todo = set(), ["embed_sets_request.h"]
    while todo:
        name = todo.pop()
        if name in seen or not (CSRC / name).exists():
            continue
        seen.add(name)
        text = (CSRC / name).read_text()
        assert "hip/hip_runtime" not in text and ".hip.h" not in re.sub(r"//.*", "", text), name
        todo += re.findall(r'#include "([^"]+)"', text)
    assert {"embed_sets_request.h", "embed_half_request.h", "embed_request.h"} <= seen


def test_what_a_restricted_table_is_made_from():
    """The module and the library exist (before this library: neither), and a node engine is refused before any native call."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed_sets import RestrictedEmbeddingTable
    assert capi.embed_sets_lib().mi355rec_embed_sets_query is not None
    _, table = ec.catalogue(40, 16)

    class Node:
        _prefix = "mi355rec_sharded_"
        _h = None

    with pytest.raises(ValueError, match="not a node engine"):
        RestrictedEmbeddingTable(Node(), table)
    with pytest.raises(ValueError, match="storage 'fp8': 'fp16' or 'bf16'"):
        RestrictedEmbeddingTable(object(), table, storage="fp8")
    with pytest.raises(ValueError, match="a fp16 table with storage='bf16'"):
        RestrictedEmbeddingTable(object(), np.ones((4, 16), np.float16), storage="bf16")
