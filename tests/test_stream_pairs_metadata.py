"""The budgets of the pair form of the streamed 8-bit scan (scan_q8_kernel_pair), read from the gfx950 code objects inside
the built library (no GPU needed: spotify_recommender_amd/build.py, kernel_metadata).

The library is at its cap of sixty kernels, so the pair form took the slot of the streamed scan's by-row instantiation
(the one streamed form tests its query pointer at run time); it must keep the occupancy the launch geometry assumes (two
workgroups of 512 threads per CU: <= 128 VGPRs, <= 80 KB of LDS, no scratch) and must not have cost the one-query streamed
kernel anything: (120 VGPRs, 44088 B of LDS) is what that kernel had in the commit before pairs (docs/LAB_NOTES.md,
"Streamed single queries: one pass per queued pair")."""
import pytest

from spotify_recommender_amd import build

PARENT_STREAMED = (120, 44088)   # (vgpr, lds) of scan_q8_kernel<Q8Cfg<512, 4, 2>, *, kWithMerge = true> before this change


@pytest.fixture(scope="module")
def kernels(engine_lib):
    return build.kernel_metadata(build.LIB_ENGINE)


def test_kernel_count_stays_within_the_cap(kernels):
    assert len(kernels) <= 60, len(kernels)


def test_the_pair_kernel_keeps_two_workgroups_per_cu(kernels):
    pair = [k for k in kernels if "scan_q8_kernel_pair" in k["name"]]
    assert len(pair) == 1, [k["name"] for k in pair]
    k = pair[0]
    assert k["vgpr"] <= 128 and k["lds"] <= 80 * 1024 and k["scratch"] == 0, k


def test_the_single_streamed_kernel_did_not_pay_for_it(kernels):
    # kWithMerge is the third template argument: "...Q8CfgILi512ELi4ELi2EEELb<row>ELb1ELb0EE..."
    streamed = [k for k in kernels if "14scan_q8_kernelI" in k["name"] and "EELb0ELb1ELb0EE" in k["name"]]
    assert len(streamed) == 1, [k["name"] for k in kernels if "scan_q8_kernel" in k["name"]]
    assert not [k for k in kernels if "14scan_q8_kernelI" in k["name"] and "EELb1ELb1ELb0EE" in k["name"]], "the by-row streamed form is back"
    k = streamed[0]
    assert k["vgpr"] <= PARENT_STREAMED[0] and k["lds"] <= PARENT_STREAMED[1] and k["scratch"] == 0, k
