"""EMBEDDING TABLES without a GPU (include/mi355rec_embed.h): a table over the node handle of the CPU placement answers
_query and _scores bit for bit as tests/embed_oracle.py states the contract; the refusals, each with its code and text;
updates of the audio rows are seen; the companion's bindings; and csrc/embed_request.h + csrc/embed_cpu.cpp as a
stand-alone program (tests/embed_check.cpp) under AddressSanitizer and UBSan, run as its own process."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import embed_cases as ec

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"
F32 = np.float32


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU placement is never taken here")


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


@cpu_only
@pytest.mark.parametrize("d", [16, 32, 64, 128])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 2049, 65537])
def test_cpu_placement_matches_the_oracle(engine_lib, n, d):
    from spotify_recommender_amd.embed import EmbeddingTable
    feats, table = ec.catalogue(n, d)
    with _node(feats) as nd, EmbeddingTable(nd, table) as tab:
        info = tab.info()
        assert (info["rows"], info["dim"], info["device"], info["tile_rows"], info["shards"]) == (n, d, -1, 0, 1)
        reqs = ec.requests(n, d)
        for i, req in enumerate(reqs):
            ec.check(tab, feats, table, req, f"n={n} d={d} request {i}")
        info = tab.info()
        assert info["queries"] == 2 * len(reqs) and info["scores_launches"] == 0


@cpu_only
def test_a_narrow_table_is_zero_padded(engine_lib):
    from spotify_recommender_amd.embed import EmbeddingTable
    n = 300
    feats, wide = ec.catalogue(n, 32)
    wide[:, 20:] = 0
    with _node(feats) as nd, EmbeddingTable(nd, wide[:, :20]) as tab:
        assert (tab.user_dim, tab.dim) == (20, 32)
        req = dict(user=wide[7, :20], metric="cosine", embed_weight=1.0, audio_weight=0.5, audio_row=3, topn=25)
        full = dict(req, user=wide[7])
        v, c, ids, sc = ec.expected(feats, wide, full)
        gi, gs = tab.query(**req)
        assert gi.tolist() == ids.tolist() and np.array_equal(gs.view(np.uint32), sc.view(np.uint32))


@cpu_only
def test_updated_audio_rows_are_seen(engine_lib):
    from spotify_recommender_amd.embed import EmbeddingTable
    n, d = 2049, 16
    feats, table = ec.catalogue(n, d)
    rng = np.random.default_rng(5)
    req = dict(rows=[4, 9, 100], metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=77, topn=50)
    with _node(feats) as nd, EmbeddingTable(nd, table) as tab:
        ec.check(tab, feats, table, req, "before the update")
        rows = [77, 0, n - 1, 500]
        new = rng.random((len(rows), 12), dtype=F32)
        feats[rows] = new
        nd.update_rows(rows, new)
        ec.check(tab, feats, table, req, "after the update")


def _raw(nd, table, dim=None, n=None):
    from spotify_recommender_amd import capi
    L = capi.embed_lib()
    e = ctypes.c_void_p()
    rc = L.mi355rec_embed_create_node(nd._h, table.ctypes.data_as(ctypes.c_void_p), table.shape[0] if n is None else n,
                                      table.shape[1] if dim is None else dim, ctypes.byref(e))
    return L, e, rc


@cpu_only
def test_refusals(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed import EmbeddingTable
    n, d = 40, 16
    feats, table = ec.catalogue(n, d)
    user = table[2].copy()
    with _node(feats) as nd:
        # create: dim 12 and 24 (the Python layer would pad them: the raw call), rows that do not match the handle
        for dim, text in ((12, b"embedding dim 12: 16, 32, 64 or 128"), (24, b"embedding dim 24: 16, 32, 64 or 128")):
            L, e, rc = _raw(nd, np.zeros((n, dim), F32))
            assert rc == capi.ERR_INVALID_ARG and not e and text in L.mi355rec_embed_last_error(None)
        L, e, rc = _raw(nd, table, n=n - 1)
        assert rc == capi.ERR_INVALID_ARG and b"table of 39 rows for a handle of 40 rows" in L.mi355rec_embed_last_error(None)
        with pytest.raises(capi.Mi355Error, match="table of 41 rows for a handle of 40 rows"):
            EmbeddingTable(nd, np.zeros((n + 1, d), F32))
        with EmbeddingTable(nd, table) as tab:
            table_of_refusals = [
                (dict(rows=list(range(33))), "33 member rows: 1 to 32 are supported"),
                (dict(rows=[]), "0 member rows: 1 to 32 are supported"),
                (dict(user=user, rows=[1]), "user by value and by rows in one embed query"),
                (dict(), "an embed query needs user by value or by rows"),
                (dict(user=user, topn=0), r"topn 0 out of \[1, 1024\]"),
                (dict(user=user, topn=1025), r"topn 1025 out of \[1, 1024\]"),
                (dict(user=user, embed_weight=0.0), "embed_weight 0: finite, not 0 and at most 4"),
                (dict(user=user, embed_weight=float("nan")), "embed_weight nan: finite, not 0 and at most 4"),
                (dict(user=user, embed_weight=float("inf")), "embed_weight inf: finite, not 0 and at most 4"),
                (dict(user=user, embed_weight=4.5), "embed_weight 4.5: finite, not 0 and at most 4"),
                (dict(user=user, audio_weight=float("-inf"), audio_row=0), "audio_weight -inf: finite and at most 4"),
                (dict(user=user, audio_weight=1.0), "audio_weight 1 needs audio by value or a valid audio_row, got row -1"),
                (dict(user=user, audio_weight=1.0, audio_row=n), "needs audio by value or a valid audio_row, got row 40"),
                (dict(user=user, exclude=list(range(1025))), r"n_exclude 1025 out of \[0, 1024\]"),
                (dict(rows=[n]), "Invalid song index: 40"),
                (dict(rows=[0, -1]), "Invalid song index: -1"),
            ]
            for kw, text in table_of_refusals:
                with pytest.raises(capi.Mi355Error, match=text) as err:
                    tab.query(**kw)
                assert err.value.code == capi.ERR_INVALID_ARG, kw
            with pytest.raises(ValueError):
                tab.query(user=user, metric="manhattan")
            # the raw structs: a wrong size, an unknown metric, flags, a null out_idx
            L = capi.embed_lib()
            q = capi.EmbedQuery(size=ctypes.sizeof(capi.EmbedQuery), user=user.ctypes.data, topn=5, w_embed=1.0)
            idx = np.empty(5, np.int64)
            res = capi.EmbedResult(size=ctypes.sizeof(capi.EmbedResult), out_idx=idx.ctypes.data)

            def refused(text):
                assert L.mi355rec_embed_query(tab._e, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG
                assert text in L.mi355rec_embed_last_error(tab._e), L.mi355rec_embed_last_error(tab._e)

            assert L.mi355rec_embed_query(tab._e, ctypes.byref(q), ctypes.byref(res)) == capi.OK
            for size in (0, 70, 76):
                q.size = size
                refused(b"embed query of size %d: not the end of a field of the 72 bytes" % size)
            q.size = 72
            res.size = 20
            refused(b"embed result of size 20: not the end of a field of the 32 bytes")
            res.size = 32
            q.metric = 2
            refused(b"metric 2 in an embed query")
            q.metric, q.flags = 0, 1
            refused(b"flags 0x1 in an embed query: must be 0")
            q.flags, res.out_idx = 0, None
            refused(b"null out_idx in an embed result")
            res.out_idx = idx.ctypes.data
            # a SHORTER struct is read as "later fields zero": w_embed missing is the zero weight's refusal
            q.size = capi.EmbedQuery.w_embed.offset
            refused(b"embed_weight 0: finite, not 0")
            q.size = 72
            assert L.mi355rec_embed_query(tab._e, ctypes.byref(q), ctypes.byref(res)) == capi.OK
            assert L.mi355rec_embed_query(None, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG
            assert L.mi355rec_embed_enqueue_probe(tab._e, ctypes.c_void_p(16), None) == capi.ERR_INVALID_ARG   # no device table here
            # every refusal left the table answering
            ec.check(tab, feats, table, ec.requests(n, d)[1], "after the refusals")


def test_the_node_accessors_refuse_what_they_do_not_serve(engine_lib):
    from spotify_recommender_amd import capi
    L = engine_lib
    out, rows, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    assert L.mi355rec_sharded_shard_handle(None, 0, ctypes.byref(out)) == capi.ERR_INVALID_ARG
    assert L.mi355rec_sharded_host_rows(None, ctypes.byref(rows), ctypes.byref(n)) == capi.ERR_INVALID_ARG
    if _gpu_visible():
        return
    feats = np.random.default_rng(1).random((9, 12), dtype=F32)
    with _node(feats) as nd:
        assert L.mi355rec_sharded_shard_handle(nd._h, 0, ctypes.byref(out)) == capi.ERR_INVALID_ARG and not out
        assert b"the CPU backend has no device shard 0" in L.mi355rec_sharded_last_error(nd._h)
        assert L.mi355rec_sharded_host_rows(nd._h, ctypes.byref(rows), ctypes.byref(n)) == capi.OK and n.value == 9
        got = np.ctypeslib.as_array(ctypes.cast(rows, ctypes.POINTER(ctypes.c_float)), shape=(9, 12))
        assert np.array_equal(got, feats)


@pytest.fixture(scope="module")
def embed_check(tmp_path_factory):
    """tests/embed_check.cpp with csrc/embed_cpu.cpp, built with AddressSanitizer and UBSan (its own process: nothing is
    preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed") / "embed_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fopenmp", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_check.cpp"), str(CSRC / "embed_cpu.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_request_h_under_sanitizers(embed_check):
    p = subprocess.run([str(embed_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_request.h: ok" in p.stdout, p.stdout + p.stderr
