"""CANDIDATE LISTS add a branch of playlist_scan_kernel and host code, not a kernel: read from the built library
(spotify_recommender_amd.build.kernel_metadata) — the five new symbols are exported, the library holds exactly 60 kernels with ONE
playlist_scan_kernel, and that kernel stays within 128 VGPRs, 80 KB of LDS and no scratch."""
from spotify_recommender_amd import build

SYMBOLS = ("mi355rec_query_playlist_request_candidates", "mi355rec_query_distance_request_candidates",
           "mi355rec_sharded_query_playlist_request_candidates", "mi355rec_sharded_query_distance_request_candidates",
           "mi355rec_candidates_counters")


def test_the_candidate_list_entry_points_are_exported(engine_lib):
    for name in SYMBOLS:
        assert hasattr(engine_lib, name), name


def test_sixty_kernels_and_one_playlist_kernel_within_its_budget(engine_lib):
    kernels = build.kernel_metadata()
    assert len(kernels) == 60, len(kernels)
    scans = [k for k in kernels if "playlist_scan_kernel" in k["name"]]
    assert len(scans) == 1, [k["name"] for k in scans]
    k = scans[0]
    print(k)
    assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] <= 80 * 1024, k
