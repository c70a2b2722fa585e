"""MANHATTAN REQUESTS add ONE kernel, manhattan_scan_kernel (csrc/anyof.hip.h: the kL1 instances of any-of's pieces in a
__global__ of their own), and take the slot of the second scores-only scan_kernel instance, whose two query forms are now one
kernel.  Read from the built library (spotify_recommender_amd.build.kernel_metadata): the two new symbols are exported, bound and
in the header; the library still holds exactly 60 kernels and none reserves scratch; there is ONE anyof_scan_kernel, ONE
playlist_scan_kernel and ONE manhattan_scan_kernel, each within 128 VGPRs and 80 KB of LDS (512 threads, two workgroups per CU:
four waves per SIMD); anyof_scan_kernel's registers and LDS are what they were before the metric existed."""
from spotify_recommender_amd import build, capi

SYMBOLS = ("mi355rec_query_manhattan_request", "mi355rec_sharded_query_manhattan_request")


def test_the_manhattan_entry_points_are_exported_and_bound(engine_lib):
    header = (build.INCLUDE / "mi355rec_diag.h").read_text()
    for name in SYMBOLS:
        assert hasattr(engine_lib, name) and name in capi.SIGNATURES and name + "(" in header, name
    for struct in ("mi355rec_manhattan_query_t", "mi355rec_manhattan_result_t"):
        assert "} " + struct + ";" in header, struct
    assert hasattr(capi, "ManhattanQuery") and hasattr(capi, "ManhattanResult")
    assert "MANHATTAN REQUESTS" in header


def test_sixty_kernels_and_the_three_scans_within_their_budget(engine_lib):
    assert all(hasattr(engine_lib, name) for name in SYMBOLS)   # (the figures below are those of a library that has the request)
    kernels = build.kernel_metadata()
    assert len(kernels) == 60, len(kernels)
    assert all(k["scratch"] == 0 for k in kernels)
    found = {}
    for fragment in ("anyof_scan_kernel", "playlist_scan_kernel", "manhattan_scan_kernel"):
        scans = [k for k in kernels if fragment in k["name"]]
        assert len(scans) == 1, [k["name"] for k in scans]
        k = found[fragment] = scans[0]
        print(k)
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] <= 80 * 1024, k
    # any-of's kernel carries nothing of the metric: its figures before the request existed
    assert (found["anyof_scan_kernel"]["vgpr"], found["anyof_scan_kernel"]["lds"]) == (100, 41_008), found["anyof_scan_kernel"]
    # the slot: the scores-only fp32 scan (kScoresOnly: no candidate list, so no LDS) is one kernel for both query forms
    scores_only = [k for k in kernels if "11scan_kernelINS_7ScanCfg" in k["name"] and k["lds"] == 0]
    assert len(scores_only) == 1 and scores_only[0]["vgpr"] <= 80, scores_only
