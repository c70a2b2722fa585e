"""MULTI-INTEREST EMBEDDING REQUESTS without a GPU (include/mi355rec_embed_multi.h): csrc/embed_multi_request.h — the
self-sized request, every refusal, and the plain statements of the value rule and of the merge of identity 2 — as a
stand-alone program (tests/embed_multi_check.cpp) under AddressSanitizer and UBSan, run as its own process; that the header
includes no HIP header; that the enqueue path of the library names no synchronise, no allocation and no copy; the numpy
statement the GPU tests use (tests/embed_multi_cases.py) against itself; and what MultiInterestEmbeddingTable refuses before
any native call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_multi_cases as mc
from tests import embed_oracle as eo
from tests.test_embed_stream_cpu import _body

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"
F32 = np.float32


@pytest.fixture(scope="module")
def embed_multi_check(tmp_path_factory):
    """tests/embed_multi_check.cpp, built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed_multi") / "embed_multi_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_multi_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_multi_request_h_under_sanitizers(embed_multi_check):
    p = subprocess.run([str(embed_multi_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_multi_request.h: ok" in p.stdout, p.stdout + p.stderr


def test_the_request_header_is_host_only():
    """embed_multi_request.h and what it includes from csrc name no HIP header (g++ compiled it above)."""
    seen, todo = set(), ["embed_multi_request.h"]
    while todo:
        name = todo.pop()
        if name in seen or not (CSRC / name).exists():
            continue
        seen.add(name)
        text = (CSRC / name).read_text()
        assert "hip/hip_runtime" not in text and ".hip.h" not in re.sub(r"//.*", "", text), name
        todo += re.findall(r'#include "([^"]+)"', text)
    assert {"embed_multi_request.h", "embed_stream_request.h", "embed_half_request.h", "embed_request.h"} <= seen


def test_an_enqueue_call_names_no_wait_no_allocation_and_no_copy():
    """The enqueue entry point and every function of embed_multi.hip it reaches: no synchronise, no hipMalloc, no hipMemcpy
    or hipMemset of any kind, no call of the shared host path that has them (dev_alloc, enqueue_inputs, device_keys); what
    they call in the product library is mi355rec_enqueue_scores alone.  Every function of the file outside create, destroy
    and info is on the list: a new one has to be put on it or the check below fails."""
    text = re.sub(r"//.*", "", (CSRC / "embed_multi.hip").read_text())
    reached = ["int mi355rec_embed_multi_enqueue_query(", "int enqueue_one(", "int order_stream(", "int record_order(", "void launch_scan(",
               "void launch_scan_rows(", "void launch_scan_as("]
    entry_bodies = _body(text, reached[0]) + _body(text, "int enqueue_one(") + _body(text, "void launch_scan(") + _body(text, "void launch_scan_rows(")
    called = set(re.findall(r"\b([a-z_]+)\(", entry_bodies)) & {m.group(1) for m in re.finditer(r"\n(?:int|void) ([a-z_]+)\(", text)}
    assert called <= {sig.split()[-1].rstrip("(") for sig in reached}, f"a function the enqueue call reaches is not held to the rules: {called}"
    defined = {m.group(1) for m in re.finditer(r"\n(?:int|void|const char\*) ([a-z0-9_]+)\(", text)}
    outside = {"init_multi_table", "create", "mi355rec_embed_multi_create_device", "mi355rec_embed_multi_create", "mi355rec_embed_multi_destroy",
               "mi355rec_embed_multi_last_error", "mi355rec_embed_multi_info"}
    assert defined - outside == {sig.split()[-1].rstrip("(") for sig in reached}, defined
    for sig in reached:
        body = _body(text, sig)
        for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMalloc", "hipFree", "dev_alloc", "enqueue_inputs",
                     "device_keys", "device_scores", "hipHostMalloc", "hipStreamQuery", "hipMemcpy", "hipMemset"):
            assert word not in body, (sig, word)
        used = set(re.findall(r"\b(mi355rec_[a-z0-9_]+)\(", body)) - {"mi355rec_embed_multi_enqueue_query"}
        assert used <= {"mi355rec_enqueue_scores", "mi355rec_last_error"}, (sig, used)
    # ... every work buffer is allocated at create
    init = _body(text, "int init_multi_table(")
    assert init.count("dev_alloc(") == 1 and "hipEventCreateWithFlags" in init
    # ... the launches of a request are the stream library's prepare, the scan, merge_kernel and the finish
    one = _body(text, "int enqueue_one(")
    assert [k for k in ("embed_stream_prepare_kernel", "launch_scan(", "merge_kernel", "embed_multi_finish_kernel") if k in one] == \
        ["embed_stream_prepare_kernel", "launch_scan(", "merge_kernel", "embed_multi_finish_kernel"]
    assert one.index("embed_stream_prepare_kernel") < one.index("mi355rec_enqueue_scores") < one.index("launch_scan(") < one.index("merge_kernel") \
        < one.index("embed_multi_finish_kernel")
    # ... and the kernels hold no inline assembly
    kernels = re.sub(r"//.*", "", (CSRC / "embed_multi.hip.h").read_text())
    assert "asm" not in kernels and "__launch_bounds__(kEmbedBlock, 4)" in kernels and "#pragma clang fp contract(off)" in kernels


def test_the_numpy_statement_of_the_value_and_of_the_merge():
    """tests/embed_multi_cases.py against itself on a small table: best() on the pointed rows; the merge of K single-interest
    top-N lists (identity 2) is the top-N by V with its interests, at every K and topn."""
    inf, nan = F32(np.inf), F32(np.nan)
    vs = np.array([[nan, inf, -0.0, 0.25, 0.5, -1.0],
                   [inf, -3e38, 0.0, 0.75, 0.5, nan],
                   [nan, nan, -1.0, 0.75, 0.25, -2.0]], F32)
    V, k = mc.best(vs)
    assert np.isnan(V[0]) and k.tolist() == [-1, 1, 0, 1, 0, 0]
    assert eo.bits(V[1:]).tolist() == eo.bits(np.array([-3e38, -0.0, 0.75, 0.5, -1.0], F32)).tolist()
    assert mc.interest_counts(2) == [1, 2, 3, 5, 32] and mc.interest_counts(8) == [1, 2, 7, 8, 9, 17, 32] and mc.interest_counts(1) == [1, 2, 3, 32]
    for n, d in ((40, 16), (300, 32)):
        feats, table = ec.catalogue(n, d)
        for K in (1, 2, 3, 5, 32):
            us = mc.interests(K, d)
            for j, topn in enumerate((1, 10, 257, n + 1)):
                req = dict(metric=("cosine", "dot")[j % 2], embed_weight=(1.0, -0.5)[(j // 2) % 2], topn=topn,
                           exclude=mc.hostile_exclusions(n, (0, 1, 1024)[j % 3]))
                if j % 2:
                    req.update(audio_weight=0.5, audio_row=n // 2)
                ids, sc, ks, vs = mc.expected(feats, table, us, req)
                singles = [ec.expected(feats, table, dict(req, user=u))[2:] for u in us]
                mi, ms, mk = mc.merge(singles, topn)
                assert mi.tolist() == ids.tolist() and np.array_equal(eo.bits(ms), eo.bits(sc)) and mk.tolist() == ks.tolist(), (n, d, K, topn)
                assert np.array_equal(eo.bits(vs[ks, ids] + F32(0)), eo.bits(sc)), "a score is its interest's v"
                if K >= 3:
                    assert 1 not in ks.tolist(), "interest 1 repeats interest 0: it is never the lowest argmax"


class _FakeTensor:
    """What MultiInterestEmbeddingTable.query looks at before any native call, without a device."""

    def __init__(self, shape, dtype="torch.float32", cuda=True, index=0):
        import torch
        self.dtype = getattr(torch, dtype.split(".")[1])
        self.shape = tuple(shape)
        self.is_cuda = cuda

        class _Device:
            pass
        self.device = _Device()
        self.device.index = index

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        raise AssertionError("a refused request reaches no native call")


def test_what_a_multi_interest_table_refuses_before_any_native_call():
    """The module, the class and the library exist (before this library: none of them); what is refused in Python."""
    import spotify_recommender_amd as pkg
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed_multi import MultiInterestEmbeddingTable
    assert pkg.MultiInterestEmbeddingTable is MultiInterestEmbeddingTable
    assert capi.embed_multi_lib().mi355rec_embed_multi_enqueue_query is not None
    _, table = ec.catalogue(40, 16)

    class Node:
        _prefix = "mi355rec_sharded_"
        _h = None

    with pytest.raises(ValueError, match="multi-interest embedding requests are served over a CosineEngine, not a node engine"):
        MultiInterestEmbeddingTable(Node(), table)
    with pytest.raises(ValueError, match=r"an embedding table is \[rows, dim\]"):
        MultiInterestEmbeddingTable(object(), np.ones(16, np.float32))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"a torch.float64 tensor on cpu: a torch table is a CUDA tensor"):
        MultiInterestEmbeddingTable(object(), torch.ones((4, 16), dtype=torch.float64))

    # a table that was never attached: query must refuse before it touches the library
    class Engine:
        device = 0

    mt = object.__new__(MultiInterestEmbeddingTable)
    mt._engine, mt.dim, mt._e, mt._lib = Engine(), 16, None, None
    with pytest.raises(ValueError, match="interests is a CUDA tensor"):
        mt.query(torch.ones((2, 16), dtype=torch.float32))                 # a host tensor
    with pytest.raises(ValueError, match="interests is a CUDA tensor"):
        mt.query(np.ones((2, 16), np.float32))
    with pytest.raises(ValueError, match="interests is a contiguous torch.float32 tensor"):
        mt.query(_FakeTensor((2, 16), "torch.float16"))                    # a wrong dtype
    with pytest.raises(ValueError, match="interests of 32 columns for a table of 16"):
        mt.query(_FakeTensor((2, 32)))                                     # a wrong dim
    with pytest.raises(ValueError, match="interests is a contiguous torch.float32 tensor of 1 or 2 dims"):
        mt.query(_FakeTensor((2, 2, 16)))
    with pytest.raises(ValueError, match="0 interests: 1 to 32"):
        mt.query(_FakeTensor((0, 16)))
    with pytest.raises(ValueError, match="33 interests: 1 to 32"):
        mt.query(_FakeTensor((33, 16)))
    with pytest.raises(ValueError, match="interests on cuda:1 for a table on cuda:0"):
        mt.query(_FakeTensor((2, 16), index=1))
    with pytest.raises(ValueError, match="metric 'l2'"):
        mt.query(_FakeTensor((2, 16)), metric="l2")
    mt._engine = None   # (nothing to close)
