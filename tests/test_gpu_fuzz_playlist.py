"""Size- and edge-case parity sweep of the playlist kernel family on the MI355X: playlist_scan_kernel (csrc/playlist.hip.h,
engine_playlist.hip.h), label_scan_kernel (csrc/labels.hip.h) and mmr_rerank_kernel (csrc/diverse.hip.h) at the catalogue
sizes their branches turn on — 1 to 5 rows (the quad tail), 63..65, 255..257 (kPlBoundRows), 2047..2049 (a tile; a second
workgroup holding one row), 4095..4097 (kAnchorRows), 8193, 65 535..65 537 (kReplicaMinRows; the pre-filter's second
workgroup) — with the 8-bit replica absent, built on demand, and AUTO; labels of 0 / 1 / 2 / 63 / 64 / 65 / 511 / 512 / 513 /
1025 rows on labels 0 .. 1023; pools larger than the catalogue.  The cases are tests/playlist_sweep_cases.py's (the CPU leg
runs a reduced list: tests/test_playlist_sweep_cpu.py).  Every check is the project's standard one: ids identical to the
Python oracles, scores (and mmr) bit-equal, the count, and -1 / 0.0 past it.

Which copy a playlist call scans: the 8-bit replica whenever the handle HAS one (mi355rec_set_replica(OFF) steers single
queries only), so "without a replica" below is a handle that never built one: fewer than 65 536 rows and never switched ON,
or created with CREATE_NO_REPLICA.  FUZZ_PLAYLIST_CASES (environment) adds random sizes; the boundary sizes always run."""
import os

import numpy as np
import pytest

from tests import playlist_sweep_cases as cases
from tests.diverse_oracle import check3
from tests.labels_oracle import check

pytestmark = pytest.mark.gpu


def _run(obj, calls, route):
    for c in calls:
        check(c.run(obj), c.want, f"{c.what} [{route}]")


def _rows_exact(eng, call):
    before = eng.playlist_counters()["rows_exact"]
    check(call.run(eng), call.want, call.what)
    return eng.playlist_counters()["rows_exact"] - before


def _sweep_catalogue(n, kind, with_lane):
    from spotify_recommender_amd import CosineEngine, capi
    name = cases.KIND_NAMES[kind]
    feats, fr, calls, more, (plain, filtered) = cases.catalogue_cases(n, kind, False)
    # ---- without a replica: every row takes the K chains, rows_exact advances by exactly n, with and without a filter
    # (the counter calls are by value with nothing excluded: a scan is launched at every size, 1, 2 and 3 rows included)
    with CosineEngine(fr, flags=capi.CREATE_NO_REPLICA if n >= 65_536 else 0) as eng:
        eng.set_replica(capi.REPLICA_OFF)
        got = _rows_exact(eng, plain)
        assert got == n, f"n={n} [{name}] no replica, no filter: rows_exact advanced by {got}"
        got = _rows_exact(eng, filtered)
        assert got == n, f"n={n} [{name}] no replica, a filter: rows_exact advanced by {got}"
        _run(eng, calls, f"{name}, replica off")
        if n < 65_536:
            # ---- the replica built on demand: the pre-filter on a handle below kReplicaMinRows
            eng.set_replica(capi.REPLICA_ON)
            _run(eng, calls, f"{name}, replica built on demand")
            if with_lane:
                lane = eng.lane()
                try:
                    _run(lane, calls[::3], f"{name}, a lane")
                finally:
                    lane.close()
    if n >= 65_536:
        with CosineEngine(fr) as eng:
            eng.set_replica(capi.REPLICA_ON)   # (OFF on this handle would launch the same: a playlist call scans a replica that exists)
            _run(eng, calls, f"{name}, replica on")
            if kind == 0 and n == 65_537:
                got = _rows_exact(eng, plain)
                print(f"rows_exact at 65 537 uniform rows, replica on, k = 3, top-10, unfiltered: {got}")
                assert 0 < got < n, f"the pre-filter did not run: rows_exact advanced by {got} of {n}"
            if with_lane:
                lane = eng.lane()
                try:
                    _run(lane, calls[::3], f"{name}, a lane")
                finally:
                    lane.close()
    if n in cases.AUTO_SIZES:
        with CosineEngine(fr) as eng:
            eng.set_replica(capi.REPLICA_AUTO)
            _run(eng, calls, f"{name}, replica AUTO")
    if more:
        with CosineEngine(feats) as eng:
            _run(eng, more, f"{name}, no ramp")
            eng.set_replica(capi.REPLICA_ON)
            _run(eng, more, f"{name}, no ramp, replica on")


@pytest.mark.parametrize("cls", list(cases.SIZE_CLASSES))
def test_playlist_sizes(engine_lib, cls):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    first = True
    for n in cases.SIZE_CLASSES[cls]:
        for kind in cases.kinds_at(n):
            _sweep_catalogue(n, kind, with_lane=first)
            first = False


def test_playlist_random_sizes(engine_lib):
    """FUZZ_PLAYLIST_CASES more sizes, drawn under FUZZ_SEED."""
    import torch  # noqa: F401
    rng = np.random.default_rng(int(os.environ.get("FUZZ_SEED", str(cases.SEED))))
    for _ in range(int(os.environ.get("FUZZ_PLAYLIST_CASES", "2"))):
        n = int(rng.choice([rng.integers(1, 300), rng.integers(300, 9000), rng.integers(9000, 70_000)], p=[.4, .4, .2]))
        _sweep_catalogue(n, int(rng.integers(0, 7)), with_lane=False)


# ---- labels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, runs", [(cases.LABEL_ROWS, cases.LABEL_RUNS), (cases.LABEL_ROWS_SMALL, cases.LABEL_RUNS_SMALL)])
def test_chosen_label_histograms(engine_lib, n, runs):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    feats, labels = cases.labelled_catalogue(n, runs)
    assert all(int((labels == lab).sum()) == c for lab, c in runs.items())
    with CosineEngine(feats) as eng:
        eng.set_labels(labels)
        cases.label_sweep(eng, feats, labels, cases.label_selections(runs), f"n={n}")
        lane = eng.lane()
        try:
            cases.label_sweep(lane, feats, labels, {"1022 and 1023": [1022, 1023]}, f"n={n}, a lane")
        finally:
            lane.close()


def test_one_label_for_every_row_and_no_label_at_all(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    for n in (513, 8193):
        feats, _ = cases.labelled_catalogue(n, {})
        one, none = np.full(n, 1023, np.int32), np.full(n, -1, np.int32)
        with CosineEngine(feats) as eng:
            eng.set_labels(one)
            cases.label_sweep(eng, feats, one, {"the label": [1023], "with empty ones": [0, 1023, 1022], "empty": [0, 1022]}, f"n={n}, one label")
            eng.set_labels(none)
            cases.label_sweep(eng, feats, none, {"any": [0], "all 1024": list(range(1024))}, f"n={n}, unlabelled")


# ---- diversified top-N on small pools ------------------------------------------------------------------------------------------
def _diverse_routes(feats, todo, what, nodes):
    """todo: [(name, call(obj) -> (ids, rel, mmr), want)] through the engine without and with the replica, a lane, and
    (nodes) a row-sharded node handle over virtual shards {0, 0, 0} and a replicated one {0, 0}."""
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_OFF)
        for name, call, want in todo:
            check3(call(eng), want, f"{what} {name} [engine, replica off]")
        eng.set_replica(capi.REPLICA_ON)
        lane = eng.lane()
        try:
            for name, call, want in todo:
                check3(call(eng), want, f"{what} {name} [engine, replica on]")
                check3(call(lane), want, f"{what} {name} [lane]")
        finally:
            lane.close()
    if nodes:
        with NodeEngine(feats, devices=[0, 0, 0], placement=capi.PLACEMENT_SHARDED) as sharded, \
                NodeEngine(feats, devices=[0, 0], placement=capi.PLACEMENT_REPLICATED) as replicated:
            assert sharded.info()["n_shards"] == 3 and sum(sharded.info()["shard_rows"]) == feats.shape[0]
            for name, call, want in todo:
                check3(call(sharded), want, f"{what} {name} [sharded {{0,0,0}}]")
                check3(call(replicated), want, f"{what} {name} [replicated {{0,0}}]")


def _todo(diverse_cases):
    return [(what, (lambda o, v=v, lam=lam, pool=pool, topn=topn: cases.run_diverse(o, v, lam, pool, topn)), want)
            for what, v, lam, pool, topn, want in diverse_cases]


@pytest.mark.parametrize("n", cases.DIVERSE_SIZES)
def test_diverse_small_pools(engine_lib, n):
    import torch  # noqa: F401
    kind, feats, todo = cases.diverse_catalogue(n)
    _diverse_routes(feats, _todo(todo), cases.KIND_NAMES[kind], nodes=n in cases.NODE_SIZES)


@pytest.mark.parametrize("name", ["1024 copies and one row", "half zero rows"])
def test_diverse_crafted_catalogues(engine_lib, name):
    """The copies: every relevance and every penalty ties, so the picks come in pool order across the sixteen waves."""
    import torch  # noqa: F401
    feats, todo = cases.crafted_diverse()[name]
    _diverse_routes(feats, _todo(todo), f"{name}:", nodes=False)


@pytest.mark.parametrize("n", cases.FETCH_SIZES)
def test_fetch_rows_on_tiny_catalogues(engine_lib, n):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = cases.catalogue_of_kind(6 if n > 4 else 3, n)
    with CosineEngine(feats) as eng:
        for rows in (list(range(n)), [n - 1, 0], [0, 0, n - 1, n // 2, n - 1, 0], list(range(n - 1, -1, -1)) * 3):
            assert np.array_equal(eng.fetch_rows(rows).view(np.uint32), feats[rows].view(np.uint32)), (n, rows[:6])
        assert eng.fetch_rows([]).shape == (0, 12)
        with pytest.raises(capi.Mi355Error) as e:
            eng.fetch_rows([n])
        assert e.value.code == capi.ERR_INVALID_ARG
        lane = eng.lane()
        try:
            assert np.array_equal(lane.fetch_rows([n - 1, 0]).view(np.uint32), feats[[n - 1, 0]].view(np.uint32))
        finally:
            lane.close()


def test_at_most_a_quarter_of_the_cases_expect_an_empty_answer():
    """Over every playlist and diversified case of this file, from the oracles' answers (no call is made here)."""
    empty, total = cases.empty_share(cpu=False)
    print(f"{empty} of {total} playlist / diversified cases expect an empty answer")
    assert total > 0 and 4 * empty <= total, f"{empty} of {total} cases expect an empty answer: more than a quarter"
