"""HALF-PRECISION EMBEDDING TABLES without a GPU (include/mi355rec_embed_half.h): to_storage and widen against torch on the
CPU, bit for bit; what HalfEmbeddingTable accepts and what it refuses before any native call; and
csrc/embed_half_request.h as a stand-alone program (tests/embed_half_check.cpp) under AddressSanitizer and UBSan, run as
its own process."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_half_cases as hc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"
F32 = np.float32


def _inputs():
    """ec.catalogue(4097, 64) (NaN, inf, 1e19, 1e-40, zero rows) plus rows of 65504, 65520, 2^-24 and 3e38."""
    _, table = ec.catalogue(4097, 64)
    extra = np.stack([np.full(64, v, F32) for v in hc.HALF_ROWS.values()])
    return np.concatenate([table, extra, -extra])


@pytest.mark.parametrize("storage", hc.STORAGES)
def test_to_storage_and_widen_are_torch_s(storage):
    import torch
    from spotify_recommender_amd.embed_half import to_storage, widen
    table = _inputs()
    dtype = torch.float16 if storage == "fp16" else torch.bfloat16
    want_t = torch.from_numpy(table).to(dtype)
    want_words = want_t.view(torch.int16).numpy().view(np.uint16)
    want_wide = want_t.to(torch.float32).numpy()
    words = to_storage(table, storage)
    assert words.dtype == np.uint16 and words.shape == table.shape
    nan = np.isnan(table)
    assert nan.any() and np.array_equal(words[~nan], want_words[~nan]), "rounding differs from torch's"
    wide = widen(words, storage)
    assert wide.dtype == np.float32 and np.array_equal(np.isnan(wide), nan), "a NaN stays a NaN, and nothing else becomes one"
    assert np.array_equal(wide[~nan].view(np.uint32), want_wide[~nan].view(np.uint32))
    assert np.array_equal(widen(want_words, storage)[~nan].view(np.uint32), want_wide[~nan].view(np.uint32))
    # the four half-specific values, by hand
    row = {v: wide[4097 + i, 0] for i, v in enumerate(hc.HALF_ROWS.values())}
    if storage == "fp16":
        assert row[F32(65504.0)] == 65504.0 and np.isinf(row[F32(65520.0)]) and row[F32(2.0 ** -24)] == F32(2.0 ** -24) and np.isinf(row[F32(3e38)])
    else:
        assert row[F32(65504.0)] == 65536.0 and row[F32(65520.0)] == 65536.0 and row[F32(2.0 ** -24)] == F32(2.0 ** -24)
        assert np.isfinite(row[F32(3e38)]) and abs(float(row[F32(3e38)]) / 3e38 - 1) < 2.0 ** -8
    # storage round-trips: narrowing the widened values gives the words back
    assert np.array_equal(to_storage(wide, storage)[~nan], words[~nan])


def test_every_word_round_trips():
    from spotify_recommender_amd.embed_half import to_storage, widen
    words = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for storage in hc.STORAGES:
        wide = widen(words, storage)
        nan = np.isnan(wide)
        assert int(nan.sum()) == (2046 if storage == "fp16" else 254)
        assert np.array_equal(to_storage(wide, storage)[~nan], words[~nan])
        assert np.isnan(widen(to_storage(wide, storage), storage)[nan]).all()


def test_what_a_half_table_is_made_from():
    """A half table can be described at all (before this library: only float32), its storage is inferred from what is
    given, and what cannot be served is refused before any native call."""
    import torch
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable, _words_of, to_storage
    assert capi.embed_half_lib().mi355rec_embed_half_create is not None
    _, table = ec.catalogue(40, 16)
    for storage, code in (("fp16", capi.EMBED_HALF_FP16), ("bf16", capi.EMBED_HALF_BF16)):
        words = to_storage(table, storage)
        for given in (hc.as_given(words, storage), torch.from_numpy(table).to(torch.float16 if storage == "fp16" else torch.bfloat16)):
            got, inferred = _words_of(given, None)
            nan = np.isnan(table)
            assert inferred == code and np.array_equal(got[~nan], words[~nan])
            assert _words_of(given, storage)[1] == code
            other = "bf16" if storage == "fp16" else "fp16"
            with pytest.raises(ValueError, match=f"a {storage} table with storage='{other}'"):
                _words_of(given, other)
        got, inferred = _words_of(table, storage)
        assert inferred == code and np.array_equal(got, words)
    with pytest.raises(ValueError, match="a float32 table needs storage='fp16' or 'bf16'"):
        _words_of(table, None)
    with pytest.raises(ValueError, match="storage 'fp8': 'fp16' or 'bf16'"):
        _words_of(table, "fp8")

    class Node:   # (what HalfEmbeddingTable asks of an engine before anything native)
        _prefix = "mi355rec_sharded_"
        _h = None

    with pytest.raises(ValueError, match="not a node engine"):
        HalfEmbeddingTable(Node(), table, storage="fp16")


def test_a_cpu_node_engine_is_refused(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    from spotify_recommender_amd.engine import NodeEngine
    if capi.lib().mi355rec_device_count() > 0:
        pytest.skip("a GPU is visible: the CPU placement is never taken here")
    feats, table = ec.catalogue(40, 16)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        with pytest.raises(ValueError, match=r"EmbeddingTable\(engine, table.widened\(\)\) answers the same bits"):
            HalfEmbeddingTable(nd, hc.as_given(hc.catalogue(40, 16, "fp16")[1], "fp16"))


@pytest.fixture(scope="module")
def embed_half_check(tmp_path_factory):
    """tests/embed_half_check.cpp, built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("embed_half") / "embed_half_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "embed_half_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_embed_half_request_h_under_sanitizers(embed_half_check):
    p = subprocess.run([str(embed_half_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "embed_half_request.h: ok" in p.stdout, p.stdout + p.stderr
