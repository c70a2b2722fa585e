"""ROW UPDATES add a job to q8_build_kernel and host code, not a kernel: read from the built library
(spotify_recommender_amd.build.kernel_metadata) — the new symbols are exported, the library still holds 60 kernels with ONE
q8_build_kernel and ONE replica_build_kernel, neither reserves scratch, and q8_build_kernel's LDS is still the 4 KiB of its
centroid job."""
from spotify_recommender_amd import build

SYMBOLS = ("mi355rec_update_rows", "mi355rec_sharded_update_rows", "mi355rec_update_info", "mi355rec_replica_entries")


def test_the_update_entry_points_are_exported(engine_lib):
    for name in SYMBOLS:
        assert hasattr(engine_lib, name), name


def test_the_builders_stay_two_kernels_within_their_budget(engine_lib):
    kernels = build.kernel_metadata()
    assert len(kernels) == 60, len(kernels)
    q8 = [k for k in kernels if "q8_build_kernel" in k["name"]]
    half = [k for k in kernels if "replica_build_kernel" in k["name"]]
    assert len(q8) == 1 and len(half) == 1, [k["name"] for k in q8 + half]
    assert q8[0]["scratch"] == 0 and half[0]["scratch"] == 0, (q8[0], half[0])
    assert q8[0]["lds"] <= 4096, q8[0]
