"""STREAMED EMBEDDING REQUESTS without a GPU (include/mi355rec_embed_stream.h): csrc/embed_stream_request.h — the two
self-sized requests, every refusal, the create checks and the plain statements of the prepare and finish steps — as a
stand-alone program (tests/embed_stream_check.cpp) under AddressSanitizer and UBSan, run as its own process; that the
header includes no HIP header; that the enqueue path of the library names no synchronise, no allocation and no blocking
copy; and what StreamedEmbeddingTable refuses before any native call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import embed_cases as ec

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


@pytest.fixture(scope="module")
def embed_stream_check(tmp_path_factory):
    """tests/embed_stream_check.cpp, built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed_stream") / "embed_stream_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_stream_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_stream_request_h_under_sanitizers(embed_stream_check):
    p = subprocess.run([str(embed_stream_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_stream_request.h: ok" in p.stdout, p.stdout + p.stderr


def test_the_request_header_is_host_only():
    """embed_stream_request.h and what it includes from csrc name no HIP header (g++ compiled it above)."""
    seen, todo = set(), ["embed_stream_request.h"]
    while todo:
        name = todo.pop()
        if name in seen or not (CSRC / name).exists():
            continue
        seen.add(name)
        text = (CSRC / name).read_text()
        assert "hip/hip_runtime" not in text and ".hip.h" not in re.sub(r"//.*", "", text), name
        todo += re.findall(r'#include "([^"]+)"', text)
    assert {"embed_stream_request.h", "embed_half_request.h", "embed_request.h"} <= seen


def _body(text, signature):
    """The braces-balanced body of the function whose definition starts with `signature`."""
    start = text.index(signature)
    i = text.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i : j + 1]
        j += 1


def test_an_enqueue_call_names_no_wait_no_allocation_and_no_blocking_copy():
    """The two enqueue entry points and every function of embed_stream.hip they reach: no synchronise, no hipMalloc, no
    hipMemcpy but the asynchronous device-to-device one, no call of the shared host path that has them (dev_alloc,
    enqueue_inputs, device_keys); what they call in the product library is mi355rec_enqueue_scores alone."""
    text = re.sub(r"//.*", "", (CSRC / "embed_stream.hip").read_text())
    reached = ["int mi355rec_embed_stream_enqueue_query(", "int mi355rec_embed_stream_enqueue_users(", "int enqueue_one(", "int enqueue_many(",
               "int order_stream(", "int record_order(", "void launch_finish(", "void launch_scan(", "void launch_scan_rows(", "void launch_scan_as(",
               "void launch_batch_scan(", "void launch_batch_scan_dim("]
    for sig in reached:
        body = _body(text, sig)
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipFree", "dev_alloc", "enqueue_inputs",
                     "device_keys", "device_scores", "hipHostMalloc", "hipStreamQuery"):
            assert word not in body, (sig, word)
        for copy in re.findall(r"hipMemcpy\w*\([^;]*;", body):
            assert copy.startswith("hipMemcpyAsync(") and "hipMemcpyDeviceToDevice" in copy, (sig, copy)
        called = set(re.findall(r"\b(mi355rec_[a-z0-9_]+)\(", body)) - {"mi355rec_embed_stream_enqueue_query", "mi355rec_embed_stream_enqueue_users"}
        assert called <= {"mi355rec_enqueue_scores", "mi355rec_last_error"}, (sig, called)
    # ... and mi355rec_enqueue_scores itself (the product library) neither waits nor copies
    engine = re.sub(r"//.*", "", (CSRC / "mi355rec.hip").read_text())
    body = _body(engine, "int mi355rec_enqueue_scores(")
    for word in ("Synchronize", "hipMalloc", "hipMemcpy"):
        assert word not in body, word


def test_what_a_streamed_table_is_made_from():
    """The module and the library exist (before this library: neither); what is refused before any native call."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    assert capi.embed_stream_lib().mi355rec_embed_stream_enqueue_query is not None
    _, table = ec.catalogue(40, 16)

    class Node:
        _prefix = "mi355rec_sharded_"
        _h = None

    with pytest.raises(ValueError, match="not a node engine"):
        StreamedEmbeddingTable(Node(), table)
    with pytest.raises(ValueError, match=r"an embedding table is \[rows, dim\]"):
        StreamedEmbeddingTable(object(), np.ones(16, np.float32))
    with pytest.raises(ValueError, match="at most 128 columns"):
        StreamedEmbeddingTable(object(), np.ones((4, 129), np.float32))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"a torch.float64 tensor on cpu: a torch table is a CUDA tensor"):
        StreamedEmbeddingTable(object(), torch.ones((4, 16), dtype=torch.float64))
