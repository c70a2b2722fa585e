"""The parity sweep of the matrix-core batch path on a host without a GPU: the cases of tests/batched_sweep_cases.py with up
to 4097 rows and 129 queries through the node handle's batch call, which the product's CPU backend serves there
(csrc/cpu_backend.cpp) — an implementation that shares nothing with the HIP kernels.  It proves the expectations of the case
module (ids, score bits, counts, padding) before the device sees them, and gives the backend of device-less hosts the same
edges: one row, topn > n, zero / tiny / huge / NaN queries, duplicate queries, mass ties."""
import pytest

from tests import batched_sweep_cases as cases


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

CASES = cases.cpu_cases()


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


@pytest.mark.parametrize("group", sorted({(c.what, c.n if c.n > 129 else 0) for c in CASES}), ids=lambda g: f"{g[0]}-{g[1] or 'le129'}")
def test_batched_sweep_through_the_cpu_backend(engine_lib, group):
    todo = [c for c in CASES if (c.what, c.n if c.n > 129 else 0) == group]
    assert todo
    for case in todo:
        q, e, _ = case.queries()
        with _node(case.feats()) as nd:
            idx, sc, counts = cases.batch_padded(nd, q, e, case.topn)
        for b in range(case.batch):
            c = int(counts[b])
            cases.check_query(case, b, idx[b, :c], sc[b, :c], q, e)


def test_the_case_lists_cover_what_they_claim():
    """No NB and no source is covered only through the exact queue; every boundary has its case."""
    got = cases.served_coverage()
    for nb in (1, 2, 4, 8, 16, 32):
        assert (nb, "fp32") in got and (nb, "replica") in got, (nb, sorted(got))
    assert {(16, "tilemax"), (32, "tilemax"), (32, "noskip")} <= got
    assert {cases.nb_of(min(b, cases.K_BQ_MAX_QUERIES)) for b in cases.BATCHES} == {1, 2, 4, 8, 16, 32}
    rows = {c.n for n in cases.ROWS for c in cases.row_cases(n)}
    assert {1, 2, 32, 64, 1024, 2048, 4096, 65_536, 131_073} <= rows
    assert all(not served for _, served in cases.edge_cases(128)[:2]) and cases.edge_cases(128)[2][1]
    assert cases.step2_rows(1280) == (5_242_880, 5_242_941)
