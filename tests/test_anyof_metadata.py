"""ANY-OF REQUESTS add ONE kernel, anyof_scan_kernel, and take the slot of half_selfcheck_kernel, which now rides in
replica_build_kernel: read from the built library (spotify_recommender_amd.build.kernel_metadata) — the two new symbols are exported,
bound and in the header, the library still holds exactly 60 kernels without scratch, ONE anyof_scan_kernel and ONE
playlist_scan_kernel, each within 128 VGPRs, 80 KB of LDS and no scratch (512 threads, two workgroups per CU)."""
from spotify_recommender_amd import build, capi

SYMBOLS = ("mi355rec_query_anyof_request", "mi355rec_sharded_query_anyof_request")


def test_the_anyof_entry_points_are_exported_and_bound(engine_lib):
    header = (build.INCLUDE / "mi355rec_diag.h").read_text()
    for name in SYMBOLS:
        assert hasattr(engine_lib, name) and name in capi.SIGNATURES and name + "(" in header, name
    for struct in ("mi355rec_anyof_query_t", "mi355rec_anyof_result_t"):
        assert "} " + struct + ";" in header, struct
    assert hasattr(capi, "AnyOfQuery") and hasattr(capi, "AnyOfResult")


def test_sixty_kernels_one_anyof_scan_and_the_playlist_kernel_within_its_budget(engine_lib):
    assert all(hasattr(engine_lib, name) for name in SYMBOLS)   # (the figures below are those of a library that has the request)
    kernels = build.kernel_metadata()
    assert len(kernels) == 60, len(kernels)
    assert all(k["scratch"] == 0 for k in kernels)
    for fragment in ("anyof_scan_kernel", "playlist_scan_kernel"):
        scans = [k for k in kernels if fragment in k["name"]]
        assert len(scans) == 1, [k["name"] for k in scans]
        k = scans[0]
        print(k)
        assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["lds"] <= 80 * 1024, k
    # the slot: the fp16 self-check is no kernel of its own any more, the replica's builder carries it
    assert not [k["name"] for k in kernels if "half_selfcheck" in k["name"]]
    assert len([k for k in kernels if "replica_build_kernel" in k["name"]]) == 1
