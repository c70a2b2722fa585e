"""JACCARD REQUESTS add NO kernel: the metric is a third value of PlaylistArg::metric, a uniform branch of playlist_row_key in
playlist_scan_kernel (csrc/playlist.hip.h, "JACCARD").  Read from the built library (spotify_recommender_amd.build.kernel_metadata):
the two new symbols are exported, bound and in the header; the library still holds exactly 60 kernels and none reserves scratch;
there is ONE playlist_scan_kernel, at exactly the 128 VGPRs and 40 128 B of LDS it had; anyof_scan_kernel and
manhattan_scan_kernel carry nothing of the metric: their registers and LDS are what they were."""
from spotify_recommender_amd import build, capi

SYMBOLS = ("mi355rec_query_jaccard_request", "mi355rec_sharded_query_jaccard_request")


def test_the_jaccard_entry_points_are_exported_and_bound(engine_lib):
    header = (build.INCLUDE / "mi355rec_diag.h").read_text()
    for name in SYMBOLS:
        assert hasattr(engine_lib, name) and name in capi.SIGNATURES and name + "(" in header, name
    for struct in ("mi355rec_jaccard_query_t", "mi355rec_jaccard_result_t"):
        assert "} " + struct + ";" in header, struct
    assert hasattr(capi, "JaccardQuery") and hasattr(capi, "JaccardResult")
    assert "JACCARD REQUESTS" in header


def test_sixty_kernels_and_the_scans_at_their_figures(engine_lib):
    assert all(hasattr(engine_lib, name) for name in SYMBOLS)   # (the figures below are those of a library that has the request)
    kernels = build.kernel_metadata()
    assert len(kernels) == 60, len(kernels)
    assert all(k["scratch"] == 0 for k in kernels), [k for k in kernels if k["scratch"] != 0]
    found = {}
    for fragment in ("anyof_scan_kernel", "playlist_scan_kernel", "manhattan_scan_kernel"):
        scans = [k for k in kernels if fragment in k["name"]]
        assert len(scans) == 1, [k["name"] for k in scans]
        found[fragment] = scans[0]
        print(scans[0])
    assert (found["playlist_scan_kernel"]["vgpr"], found["playlist_scan_kernel"]["lds"]) == (128, 40_128), found["playlist_scan_kernel"]
    assert (found["anyof_scan_kernel"]["vgpr"], found["anyof_scan_kernel"]["lds"]) == (100, 41_008), found["anyof_scan_kernel"]
    assert (found["manhattan_scan_kernel"]["vgpr"], found["manhattan_scan_kernel"]["lds"]) == (108, 39_736), found["manhattan_scan_kernel"]
