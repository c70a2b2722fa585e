"""CANDIDATE SCORES add a mode of playlist_scan_kernel's gather branch and host code, not a kernel: read from the built library
(spotify_recommender_amd.build.kernel_metadata) — the four new symbols are exported, and the library that exports them still holds
exactly 60 kernels with ONE playlist_scan_kernel within 128 VGPRs, 80 KB of LDS and no scratch."""
from spotify_recommender_amd import build, capi

SYMBOLS = ("mi355rec_score_playlist_request_candidates", "mi355rec_score_distance_request_candidates",
           "mi355rec_sharded_score_playlist_request_candidates", "mi355rec_sharded_score_distance_request_candidates")


def test_the_candidate_scores_entry_points_are_exported_and_bound(engine_lib):
    header = (build.INCLUDE / "mi355rec_diag.h").read_text()
    for name in SYMBOLS:
        assert hasattr(engine_lib, name) and name in capi.SIGNATURES and name + "(" in header, name


def test_the_library_with_the_score_mode_keeps_sixty_kernels_and_the_playlist_kernel_its_budget(engine_lib):
    assert all(hasattr(engine_lib, name) for name in SYMBOLS)   # (the figures below are those of a library that has the mode)
    kernels = build.kernel_metadata()
    assert len(kernels) == 60, len(kernels)
    scans = [k for k in kernels if "playlist_scan_kernel" in k["name"]]
    assert len(scans) == 1, [k["name"] for k in scans]
    k = scans[0]
    print(k)
    assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] <= 80 * 1024, k
