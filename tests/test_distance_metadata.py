"""DISTANCE REQUESTS add no kernel and keep playlist_scan_kernel inside its occupancy budget: read from the gfx950 code
objects inside the library that ships (spotify_recommender_amd/build.py kernel_metadata; no GPU needed)."""
import pytest

from spotify_recommender_amd import build


@pytest.fixture(scope="module")
def kernels(engine_lib):
    return build.kernel_metadata(build.LIB_ENGINE)


def _one(kernels, fragment):
    hits = [k for k in kernels if fragment in k["name"]]
    assert len(hits) == 1, (fragment, [k["name"] for k in hits])
    return hits[0]


def test_the_metric_is_a_branch_not_a_kernel(kernels, engine_lib):
    assert len(kernels) <= 60, len(kernels)
    assert hasattr(engine_lib, "mi355rec_query_distance_request") and hasattr(engine_lib, "mi355rec_sharded_query_distance_request")
    # the two kernels the feature touches are still ONE instantiation each
    _one(kernels, "playlist_scan_kernel")
    _one(kernels, "q8_build_kernel")


def test_the_playlist_kernel_keeps_two_workgroups_per_cu(kernels):
    """512 threads, two workgroups per CU (PlaylistCfg): at most 128 VGPRs and half the LDS, no scratch."""
    k = _one(kernels, "playlist_scan_kernel")
    assert k["vgpr"] <= 128 and k["lds"] <= 80 * 1024 and k["scratch"] == 0, k
