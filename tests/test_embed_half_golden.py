"""The recorded cross-backend answers of the HALF-PRECISION tables: the fp32 library's CPU placement answers for any fp32
table, so its answers for W(to_storage(table)), both storages, every request of tests/embed_cases.requests, are recorded
in tests/golden/embed_half_cpu_answers.npz (ids and score bits only).  The CPU placement must reproduce them here, and
tests/test_gpu_embed_half.py holds libmi355rec_embed_half.so's answers on the GPU against the same file — so the half
kernels are compared with the host statement of the contract although no machine runs both."""
import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_half_cases as hc
from tests import embed_oracle as eo

GOLDEN_CASE = (2049, 32)   # rows, dim


def golden_answers(golden_dir):
    return np.load(golden_dir / "embed_half_cpu_answers.npz")


def golden_words(storage):
    """The half table of the recorded case: ec.catalogue's table rounded to `storage`."""
    from spotify_recommender_amd.embed_half import to_storage
    n, d = GOLDEN_CASE
    feats, table = ec.catalogue(n, d)
    return feats, to_storage(table, storage)


def cpu_answers():
    """What the CPU placement answers now for the widened tables (how the file was recorded)."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_half import widen
    from spotify_recommender_amd.engine import NodeEngine
    n, d = GOLDEN_CASE
    out = {}
    for storage in hc.STORAGES:
        feats, words = golden_words(storage)
        with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd, EmbeddingTable(nd, widen(words, storage)) as tab:
            assert nd.placement() == capi.PLACEMENT_CPU
            for i, req in enumerate(ec.requests(n, d)):
                ids, sc = tab.query(**req)
                out[f"{storage}_ids{i}"] = ids
                out[f"{storage}_score_bits{i}"] = eo.bits(sc).copy()
    return out


def test_cpu_placement_reproduces_the_recorded_answers(engine_lib, golden_dir):
    from spotify_recommender_amd import capi
    if capi.lib().mi355rec_device_count() > 0:
        pytest.skip("a GPU is visible: the CPU placement is never taken here")
    want = golden_answers(golden_dir)
    got = cpu_answers()
    assert sorted(got) == sorted(want.files)
    for name, arr in got.items():
        assert np.array_equal(arr, want[name]), name
