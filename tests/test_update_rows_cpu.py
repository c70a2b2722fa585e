"""ROW UPDATES without a GPU (include/mi355rec_diag.h): the node handle served by the CPU backend rewrites its host matrix and
answers every route from the updated rows (tests/update_rows_cases.py: the existing oracles on the updated numpy matrix, ids
and score bits equal); the refusals leave it as it was; Recommender::updateSongs through the shim; the new symbols are
exported and bound; and csrc/rows_update.h itself as a stand-alone program (tests/update_rows_check.cpp) under AddressSanitizer
and UBSan, run as its own process."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle
from tests.playlist_labels_oracle import uniform_labels
from tests.update_rows_cases import adversarial_steps, catalogue, check_routes, new_rows, update_lists

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


@cpu_only
@pytest.mark.parametrize("n", [1, 9, 4097])
def test_updates_on_the_cpu_backend(engine_lib, n):
    from spotify_recommender_amd import capi
    cur = catalogue(n)
    rng = np.random.default_rng(n + 1)
    labels, priors = uniform_labels(n, 6, n), np.random.default_rng(n).random(n, dtype=np.float32)
    q = n // 3
    with _node(cur) as nd:
        nd.set_labels(labels)
        nd.set_priors(priors)
        for name, rows in update_lists(n, rng).items():
            new = new_rows(cur, rows, q, rng)
            t = nd.enqueue_row(q, 10)                     # a ticket from before the update: computed from the old rows, still readable
            old = oracle.topn_canonical(oracle.scores(cur, cur[q]), q, 10)
            cur[rows] = new
            nd.update_rows(rows, new)
            got = nd.wait(t, 10)
            assert got[0].tolist() == old[0].tolist()
            check_routes(nd, cur, q, f"n={n} {name}", labels, priors)
        for name, rows, new in adversarial_steps(cur, q, 1 if n < 16 else 10, rng):
            cur[rows] = new
            nd.update_rows(rows, new)
            check_routes(nd, cur, q, f"n={n} {name}", labels, priors, batches=(12,))
        nd.update_rows([], np.empty((0, 12), np.float32))   # count == 0 succeeds
        # the refusals, each leaving the handle answering as before
        for bad in ([0, 0], [n], [-1], [n - 1, n - 1, 0]):
            with pytest.raises(capi.Mi355Error) as e:
                nd.update_rows(bad, rng.random((len(bad), 12), dtype=np.float32))
            assert e.value.code == capi.ERR_INVALID_ARG
        with pytest.raises(capi.Mi355Error) as e:
            nd.update_rows([0], None)                     # NULL rows on a node handle
        assert e.value.code == capi.ERR_INVALID_ARG
        check_routes(nd, cur, q, f"n={n} after the refused calls", labels, priors, batches=(2,))


@pytest.fixture(scope="module")
def shim(engine_lib):
    from spotify_recommender_amd import build
    build.build_shim()
    L = ctypes.CDLL(str(build.LIB_SHIM))
    L.shim_from_matrix.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    L.shim_from_matrix.restype = ctypes.c_void_p
    L.shim_free.argtypes = [ctypes.c_void_p]
    L.shim_initialize.argtypes = [ctypes.c_void_p]
    L.shim_recommend_by_index.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.shim_recommend_by_index.restype = ctypes.c_int64
    L.shim_update_songs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]
    L.shim_update_songs.restype = ctypes.c_int
    return L


def _recommend(shim, h, q, topn):
    idx, sc = np.empty(topn, np.int32), np.empty(topn, np.float32)
    c = shim.shim_recommend_by_index(h, q, topn, idx.ctypes.data, sc.ctypes.data, topn)
    return idx[:c].astype(np.int64), sc[:c]


@cpu_only
def test_update_songs_through_the_shim(shim, capfd):
    n, q = 4097, 1234
    cur = catalogue(n)
    rng = np.random.default_rng(11)
    h = shim.shim_from_matrix(cur.ctypes.data, n)
    assert h
    try:
        assert shim.shim_initialize(h) == 1

        def update(rows, feats):
            r = np.asarray(rows, np.int32)
            f = np.ascontiguousarray(feats, np.float32)
            return shim.shim_update_songs(h, r.ctypes.data, r.size, f.ctypes.data, f.size)

        def check(what):
            want = oracle.topn_canonical(oracle.scores(cur, cur[q]), q, 10)
            idx, sc = _recommend(shim, h, q, 10)
            assert idx.tolist() == want[0].tolist(), what
            assert np.array_equal((sc + np.float32(0)).view(np.uint32), (want[1] + np.float32(0)).view(np.uint32)), what

        check("before any update")
        far = int(oracle.topn_canonical(oracle.scores(cur, cur[q]), q, n)[0][-1])
        rows = [far, 0, n - 1]
        new = rng.random((3, 12), dtype=np.float32)
        new[0] = cur[q]                                   # a far song becomes a copy of the query: it must come first
        cur[rows] = new
        assert update(rows, new) == 1
        check("after updateSongs")
        assert far in _recommend(shim, h, q, 10)[0].tolist()
        assert update([], np.empty((0, 12), np.float32)) == 1
        # refused: the catalogue stays as it was
        assert update([5, 5], rng.random((2, 12), dtype=np.float32)) == 0
        assert update([n], rng.random((1, 12), dtype=np.float32)) == 0
        assert update([-1], rng.random((1, 12), dtype=np.float32)) == 0
        assert update([1, 2], rng.random((1, 12), dtype=np.float32)) == 0       # a wrong length
        check("after the refused updates")
        assert "Error" in capfd.readouterr().err
    finally:
        shim.shim_free(h)


def test_the_new_symbols_are_exported_and_bound(engine_lib):
    from spotify_recommender_amd import capi
    for name in ("mi355rec_update_rows", "mi355rec_sharded_update_rows", "mi355rec_update_info", "mi355rec_replica_entries"):
        assert name in capi.SIGNATURES, name
        assert getattr(engine_lib, name).argtypes == capi.SIGNATURES[name][1], name
    assert ctypes.sizeof(capi.UpdateInfo) == 32
    assert [f[0] for f in capi.UpdateInfo._fields_] == ["size", "last_ms", "calls", "rows", "rows_since_snapshot"]
    assert capi.UpdateInfo.calls.offset == 8 and capi.UpdateInfo.rows_since_snapshot.offset == 24


@pytest.fixture(scope="module")
def update_rows_check(tmp_path_factory):
    """tests/update_rows_check.cpp built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("update_rows") / "update_rows_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           str(ROOT / "tests" / "update_rows_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_rows_update_h_under_sanitizers(update_rows_check):
    p = subprocess.run([str(update_rows_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "rows_update.h: ok" in p.stdout, p.stdout + p.stderr
