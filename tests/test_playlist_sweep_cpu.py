"""The size- and edge-case sweep of the playlist kernel family on a host without a GPU: a reduced list of the cases of
tests/playlist_sweep_cases.py (sizes up to 4097 rows, one kind each) through the node handle, which the product's CPU
backend serves there (csrc/cpu_backend.cpp).  It keeps the case generators and the oracles honest where no device is, and
gives the backend of device-less hosts the same edges: 1 to 5 rows, everything excluded, filters that admit nothing or the
last three rows, labels of 0 / 1 / 511 / 512 / 513 / 1025 rows up to label 1023, pools larger than the catalogue.
Identical ids, bit-equal scores and mmr, the count and the padding past it."""
import numpy as np
import pytest

from tests import playlist_sweep_cases as cases
from tests.diverse_oracle import check3
from tests.labels_oracle import check


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


@pytest.mark.parametrize("n, kind", cases.sweep_catalogues(cpu=True))
def test_playlist_sizes(engine_lib, n, kind):
    from spotify_recommender_amd import capi
    feats, fr, calls, more, _ = cases.catalogue_cases(n, kind, True)
    with _node(fr) as nd:
        for c in calls:
            check(c.run(nd), c.want, f"{c.what} [{cases.KIND_NAMES[kind]}]")
        with pytest.raises(capi.Mi355Error, match="out of the catalogue") as e:   # (the single-device handle lets it match nothing)
            nd.query_mean_topn(fr[:1], 1, [n])
        assert e.value.code == capi.ERR_INVALID_ARG
    if more:
        with _node(feats) as nd:
            for c in more:
                check(c.run(nd), c.want, f"{c.what} [{cases.KIND_NAMES[kind]}]")


@pytest.mark.parametrize("n, runs", [(cases.LABEL_ROWS_SMALL, cases.LABEL_RUNS_SMALL), (4097, {k: min(v, 600) for k, v in cases.LABEL_RUNS.items()})])
def test_chosen_label_histograms(engine_lib, n, runs):
    """(8193 rows with the full histogram run on the GPU; here 65 rows, and 4097 with the runs up to 600 rows.)"""
    feats, labels = cases.labelled_catalogue(n, runs)
    with _node(feats) as nd:
        nd.set_labels(labels)
        cases.label_sweep(nd, feats, labels, cases.label_selections(runs), f"n={n}")


def test_one_label_for_every_row_and_no_label_at_all(engine_lib):
    feats, _ = cases.labelled_catalogue(513, {})
    one, none = np.full(513, 1023, np.int32), np.full(513, -1, np.int32)
    with _node(feats) as nd:
        nd.set_labels(one)
        cases.label_sweep(nd, feats, one, {"the label": [1023], "with empty ones": [0, 1023, 1022], "empty": [0, 1022]}, "one label")
        nd.set_labels(none)
        cases.label_sweep(nd, feats, none, {"any": [0], "all 1024": list(range(1024))}, "unlabelled")


@pytest.mark.parametrize("n", [n for n in cases.DIVERSE_SIZES if n <= cases.CPU_MAX_ROWS])
def test_diverse_small_pools(engine_lib, n):
    kind, feats, todo = cases.diverse_catalogue(n)
    with _node(feats) as nd:
        for what, v, lam, pool, topn, want in todo:
            check3(cases.run_diverse(nd, v, lam, pool, topn), want, f"{what} [{cases.KIND_NAMES[kind]}]")


@pytest.mark.parametrize("name", ["1024 copies and one row", "half zero rows"])
def test_diverse_crafted_catalogues(engine_lib, name):
    feats, todo = cases.crafted_diverse()[name]
    with _node(feats) as nd:
        for what, v, lam, pool, topn, want in todo:
            check3(cases.run_diverse(nd, v, lam, pool, topn), want, f"{name}: {what}")


def test_at_most_a_quarter_of_the_cases_expect_an_empty_answer():
    """Over every playlist and diversified case of this file, from the oracles' answers (no call is made here)."""
    empty, total = cases.empty_share(cpu=True)
    print(f"{empty} of {total} playlist / diversified cases expect an empty answer")
    assert total > 0 and 4 * empty <= total, f"{empty} of {total} cases expect an empty answer: more than a quarter"
