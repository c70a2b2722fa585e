"""EMBEDDING CANDIDATE LISTS without a GPU (include/mi355rec_embed_cand.h): csrc/embed_cand_request.h — the self-sized
request, every refusal, and the plain statements of the id mapping and of the claim — as a stand-alone program
(tests/embed_cand_check.cpp) under AddressSanitizer and UBSan, run as its own process; that the header includes no HIP
header; that the enqueue path of the library names no synchronise, no allocation and no blocking copy; and what
CandidateEmbeddingTable refuses before any native call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import embed_cases as ec
from tests.test_embed_stream_cpu import _body

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


@pytest.fixture(scope="module")
def embed_cand_check(tmp_path_factory):
    """tests/embed_cand_check.cpp, built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed_cand") / "embed_cand_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_cand_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_cand_request_h_under_sanitizers(embed_cand_check):
    p = subprocess.run([str(embed_cand_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_cand_request.h: ok" in p.stdout, p.stdout + p.stderr


def test_the_request_header_is_host_only():
    """embed_cand_request.h and what it includes from csrc name no HIP header (g++ compiled it above)."""
    seen, todo = set(), ["embed_cand_request.h"]
    while todo:
        name = todo.pop()
        if name in seen or not (CSRC / name).exists():
            continue
        seen.add(name)
        text = (CSRC / name).read_text()
        assert "hip/hip_runtime" not in text and ".hip.h" not in re.sub(r"//.*", "", text), name
        todo += re.findall(r'#include "([^"]+)"', text)
    assert {"embed_cand_request.h", "embed_stream_request.h", "embed_half_request.h", "embed_request.h"} <= seen


def test_an_enqueue_call_names_no_wait_no_allocation_and_no_blocking_copy():
    """The two enqueue entry points and every function of embed_cand.hip they reach: no synchronise, no hipMalloc, no
    hipMemcpy or hipMemset of any kind, no call of the shared host path that has them (dev_alloc, enqueue_inputs,
    device_keys); what they call in the product library is mi355rec_enqueue_scores alone.  Every function of the file
    outside create, destroy and info is on the list: a new one has to be put on it or the count below fails."""
    text = re.sub(r"//.*", "", (CSRC / "embed_cand.hip").read_text())
    reached = ["int mi355rec_embed_cand_enqueue_rank(", "int mi355rec_embed_cand_enqueue_scores(", "int enqueue_rank(", "int enqueue_values(",
               "int enqueue_audio(", "EmbedArgs gather_args(", "int order_stream(", "int record_order(", "int tile_entries(", "void launch_gather(",
               "void launch_gather_rows(", "void launch_gather_as("]
    entry_bodies = _body(text, reached[0]) + _body(text, reached[1]) + _body(text, "int enqueue_rank(") + _body(text, "int enqueue_values(")
    called = set(re.findall(r"\b([a-z_]+)\(", entry_bodies)) & {m.group(1) for m in re.finditer(r"\n(?:int|void|EmbedArgs) ([a-z_]+)\(", text)}
    assert called <= {sig.split()[-1].rstrip("(") for sig in reached}, f"a function the enqueue calls reach is not held to the rules: {called}"
    for sig in reached:
        body = _body(text, sig)
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipFree", "dev_alloc", "enqueue_inputs",
                     "device_keys", "device_scores", "hipHostMalloc", "hipStreamQuery", "hipMemcpy", "hipMemset"):
            assert word not in body, (sig, word)
        used = set(re.findall(r"\b(mi355rec_[a-z0-9_]+)\(", body)) - {"mi355rec_embed_cand_enqueue_rank", "mi355rec_embed_cand_enqueue_scores"}
        assert used <= {"mi355rec_enqueue_scores", "mi355rec_last_error"}, (sig, used)
    # ... every work buffer is allocated at create, and the claim bitmap is zeroed there
    init = _body(text, "int init_cand_table(")
    assert init.count("dev_alloc(") == 3 and "hipMemset(e->d_claim, 0" in init and "hipEventCreateWithFlags" in init
    # ... and the kernels hold no inline assembly
    kernels = re.sub(r"//.*", "", (CSRC / "embed_cand.hip.h").read_text())
    assert "asm" not in kernels and "__launch_bounds__(kEmbedBlock, 4)" in kernels


def test_what_a_candidate_table_is_made_from():
    """The module and the library exist (before this library: neither); what is refused before any native call."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed_cand import CandidateEmbeddingTable
    assert capi.embed_cand_lib().mi355rec_embed_cand_enqueue_rank is not None
    _, table = ec.catalogue(40, 16)

    class Node:
        _prefix = "mi355rec_sharded_"
        _h = None

    with pytest.raises(ValueError, match="embedding candidate lists are served over a CosineEngine, not a node engine"):
        CandidateEmbeddingTable(Node(), table)
    with pytest.raises(ValueError, match=r"an embedding table is \[rows, dim\]"):
        CandidateEmbeddingTable(object(), np.ones(16, np.float32))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"a torch.float64 tensor on cpu: a torch table is a CUDA tensor"):
        CandidateEmbeddingTable(object(), torch.ones((4, 16), dtype=torch.float64))
    # ... and the streamed table it shares its attachment with says what it said
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    with pytest.raises(ValueError, match="streamed embedding requests are served over a CosineEngine, not a node engine"):
        StreamedEmbeddingTable(Node(), table)
