"""The CPU placement's answers for one catalogue, recorded in tests/golden/embed_cpu_answers.npz (ids and score bits of
every request of tests/embed_cases.requests): the CPU placement must reproduce them here, and tests/test_gpu_embed.py
holds the GPU's answers against the same file — so the two backends are compared although no machine runs both."""
import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_oracle as eo

GOLDEN_CASE = (2049, 32)   # rows, dim


def golden_answers(golden_dir):
    return np.load(golden_dir / "embed_cpu_answers.npz")


def cpu_answers():
    """What the CPU placement answers now (how the file was recorded)."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.engine import NodeEngine
    n, d = GOLDEN_CASE
    feats, table = ec.catalogue(n, d)
    out = {}
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd, EmbeddingTable(nd, table) as tab:
        assert nd.placement() == capi.PLACEMENT_CPU
        for i, req in enumerate(ec.requests(n, d)):
            ids, sc = tab.query(**req)
            out[f"ids{i}"] = ids
            out[f"score_bits{i}"] = eo.bits(sc).copy()
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
