"""USER BATCHES without a GPU (include/mi355rec_embed_batch.h): csrc/embed_batch_request.h — the argument checks, each
refusal with its text, and the exclusion lists as the scan wants them — as a stand-alone program
(tests/embed_batch_check.cpp) under AddressSanitizer and UBSan, run as its own process; and what the library refuses
before it needs a device."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"
F32 = np.float32


@pytest.fixture(scope="module")
def batch_check(tmp_path_factory):
    """tests/embed_batch_check.cpp, built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed_batch") / "embed_batch_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_batch_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_batch_request_h_under_sanitizers(batch_check):
    p = subprocess.run([str(batch_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_batch_request.h: ok" in p.stdout, p.stdout + p.stderr


def test_create_refuses_a_null_handle_and_a_null_out():
    from spotify_recommender_amd import build, capi
    build.build_embed_batch()
    L = capi.embed_batch_lib()
    table = np.zeros((4, 16), F32)
    e = ctypes.c_void_p()
    assert L.mi355rec_embed_batch_create(None, table.ctypes.data_as(ctypes.c_void_p), 4, 16, ctypes.byref(e)) == capi.ERR_INVALID_ARG
    assert not e and b"null argument" in L.mi355rec_embed_batch_last_error(None)
    assert L.mi355rec_embed_batch_create(ctypes.c_void_p(16), table.ctypes.data_as(ctypes.c_void_p), 4, 16, None) == capi.ERR_INVALID_ARG


def test_the_python_layer_checks_shapes_before_the_library():
    """What EmbeddingBatchTable.query_users refuses on its own needs no table: the checks stand ahead of the native call."""
    from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
    tab = EmbeddingBatchTable.__new__(EmbeddingBatchTable)
    tab.user_dim, tab.dim, tab.rows = 20, 32, 5
    tab._table = np.arange(5 * 32, dtype=F32).reshape(5, 32)
    tab._engine = None
    tab._e = None
    with pytest.raises(ValueError, match="'cosine' or 'dot'"):
        tab.query_users(users=np.zeros((1, 20), F32), metric="manhattan")
    with pytest.raises(ValueError, match="by value or by rows"):
        tab.query_users()
    with pytest.raises(ValueError, match="by value or by rows"):
        tab.query_users(users=np.zeros((1, 20), F32), rows=[[1]])
    with pytest.raises(ValueError, match=r"users of shape \(1, 21\)"):
        tab.query_users(users=np.zeros((1, 21), F32))
    with pytest.raises(ValueError, match="2 exclusion lists for 1 users"):
        tab.query_users(users=np.zeros((1, 20), F32), exclude=[[1], [2]])
    with pytest.raises(ValueError, match="Invalid song index: 5"):
        tab.query_users(rows=[[0, 5]])
    with pytest.raises(ValueError, match="0 member rows"):
        tab.query_users(rows=[[1], []])
    # the in-order float32 sums of the contract (tests/embed_oracle.user_from_rows states them)
    from tests import embed_oracle as eo
    got = tab._users_from_rows([[4, 0, 2], [3]])
    assert np.array_equal(got[0], eo.user_from_rows(tab._table, [4, 0, 2])) and np.array_equal(got[1], tab._table[3])
