"""LABELS on the MI355X: label-filtered top-N (csrc/labels.hip.h, label_scan_kernel over the label-grouped rows of
csrc/engine_labels.hip.h) checked bit for bit against the oracle restricted to the selected rows; the rows the launches
scan; unfiltered queries unchanged by labels; lanes; the node handle (virtual shards, replicas); the C++ drop-in."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import catalogue, check, expected, expected_from_scores

pytestmark = pytest.mark.gpu

SETS = {
    "one": [7],
    "two": [3, 5],
    "alternating": list(range(0, 114, 2)),
    "all": list(range(114)),
    "empty label": [500],
    "duplicates": [5, 5, 3, 5],
}


@pytest.fixture(scope="module")
def uniform_1m(engine_lib):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine
    feats, labels = catalogue(1_000_000, 114, seed=21)
    eng = CosineEngine(feats)
    eng.set_labels(labels)
    yield eng, feats, labels
    eng.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_1m_uniform_matches_the_oracle(uniform_1m, name):
    eng, feats, labels = uniform_1m
    wanted = SETS[name]
    member = np.isin(labels, wanted)
    selected = int(member.sum())
    inside = [r for r in (99, 10, 200) if member[r]] or ([int(np.flatnonzero(member)[0])] if selected else [])
    outside = [int(np.flatnonzero(~member)[0]), 999_999 if not member[999_999] else int(np.flatnonzero(~member)[-1])]
    for q in inside + outside:
        scores = oracle.scores(feats, feats[q])
        for topn in (1, 10, 100, 1024, 1500, selected + 5):
            want = expected_from_scores(scores, labels, q, wanted, topn)
            check(eng.query_row_topn_labels(q, wanted, topn), want, f"{name} row {q} top-{topn}")
        # by value: nothing excluded, and the row excluded by its global index
        for excl in (-1, q):
            want = expected_from_scores(scores, labels, excl, wanted, 100)
            check(eng.query_topn_labels(feats[q], excl, wanted, 100), want, f"{name} by value, exclude {excl}")
    vec = np.random.default_rng(2).random(12, dtype=np.float32)
    check(eng.query_topn_labels(vec, -1, wanted, 1500), expected(feats, labels, vec, -1, wanted, 1500), f"{name} vector")


def test_one_label_scans_only_its_rows(uniform_1m):
    eng, feats, labels = uniform_1m
    before = eng.label_counters()
    eng.query_row_topn_labels(0, [42], 10)
    after = eng.label_counters()
    rows = int((labels == 42).sum())
    assert after["queries"] - before["queries"] == 1
    scanned = after["rows_scanned"] - before["rows_scanned"]
    assert rows <= scanned <= (rows + 511) // 512 * 512 and scanned < labels.size // 50, (rows, scanned)


def test_unfiltered_results_are_unchanged_by_labels(engine_lib):
    from spotify_recommender_amd import CosineEngine
    feats, labels = catalogue(1_000_000, 114, seed=31)
    rows = (np.arange(50, dtype=np.int64) * 19_997) % feats.shape[0]

    def run(eng):
        st0 = eng.stats()
        out = [eng.query_row_topn(int(r), 100) for r in rows]
        st1 = eng.stats()
        moved = {f: getattr(st1, f) - getattr(st0, f) for f, _ in type(st0)._fields_ if f.startswith("route_")}
        return out, moved

    with CosineEngine(feats) as eng:
        before, moved_before = run(eng)
        eng.set_labels(labels)
        after, moved_after = run(eng)
    for (bi, bs), (ai, as_) in zip(before, after):
        assert bi.tolist() == ai.tolist() and np.array_equal(bs.view(np.uint32), as_.view(np.uint32))
    assert moved_before == moved_after, (moved_before, moved_after)


def test_10m_genre_contiguous(engine_lib):
    import torch
    from spotify_recommender_amd import CosineEngine
    n = 10_000_000
    feats = oracle.mt19937_uniform(77, n)
    labels = (np.arange(n, dtype=np.int64) * 114 // n).astype(np.int32)     # blocks, as a preprocessed CSV is grouped
    dev = torch.from_numpy(feats).to("cuda:0")
    with CosineEngine(dev) as eng:
        eng.set_labels(labels)
        rng = np.random.default_rng(9)
        for size in (1, 8, 57, 114):
            wanted = sorted(rng.choice(114, size=size, replace=False).tolist())
            for q in (int(rng.integers(n)), int(np.flatnonzero(labels == wanted[0])[3])):
                scores = oracle.scores(feats, feats[q])
                for topn in (10, 100):
                    check(eng.query_row_topn_labels(q, wanted, topn), expected_from_scores(scores, labels, q, wanted, topn),
                          f"{size} labels, row {q}, top-{topn}")


def test_lanes_share_the_labels(engine_lib):
    from spotify_recommender_amd import CosineEngine, capi
    feats, labels = catalogue(300_000, 114, seed=41)
    parent = CosineEngine(feats)
    parent.set_labels(labels)
    lane = parent.lane()
    try:
        for q, wanted in ((5, [1]), (77, [3, 5, 9]), (1234, list(range(114)))):
            a = parent.query_row_topn_labels(q, wanted, 50)
            b = lane.query_row_topn_labels(q, wanted, 50)
            check(b, a, "lane")
            check(a, expected(feats, labels, feats[q], q, wanted, 50), "parent")
        with pytest.raises(capi.Mi355Error, match="lanes"):
            parent.set_labels(labels)
        with pytest.raises(capi.Mi355Error, match="lanes"):
            lane.set_labels(None)
        parent.close()   # the group keeps the labels while the lane lives
        check(lane.query_row_topn_labels(77, [3, 5, 9], 50), expected(feats, labels, feats[77], 77, [3, 5, 9], 50), "lane alone")
    finally:
        lane.close()
        parent.close()


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handle_matches_the_single_handle(engine_lib, placement):
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, labels = catalogue(400_000, 114, seed=51)
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    with CosineEngine(feats) as single, NodeEngine(feats, devices=[0, 0], placement=pl) as node:
        single.set_labels(labels)
        node.set_labels(labels)
        assert node.info()["n_shards"] == 2
        for q, wanted in ((0, [7]), (99, [5]), (250_000, [3, 5]), (399_999, list(range(0, 114, 2)))):
            for topn in (10, 1500):
                want = single.query_row_topn_labels(q, wanted, topn)
                check(want, expected(feats, labels, feats[q], q, wanted, topn), f"single row {q}")
                check(node.query_row_topn_labels(q, wanted, topn), want, f"{placement} row {q} top-{topn}")
            check(node.query_topn_labels(feats[q], -1, wanted, 20), single.query_topn_labels(feats[q], -1, wanted, 20),
                  f"{placement} by value")
        node.set_labels(None)
        with pytest.raises(capi.Mi355Error, match="no labels"):
            node.query_row_topn_labels(0, [7], 10)


def test_recommender_in_genres_on_the_114k_csv(tmp_path):
    import torch  # noqa: F401
    from spotify_recommender_amd import build, capi
    from tests.test_cpu_backend import _config1_csv
    capi.lib()
    build.build_shim()
    L = ctypes.CDLL(str(build.LIB_SHIM))
    L.shim_preprocess.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.shim_load.argtypes = [ctypes.c_char_p]
    L.shim_load.restype = ctypes.c_void_p
    for name in ("shim_free", "shim_initialize"):
        getattr(L, name).argtypes = [ctypes.c_void_p]
    L.shim_song_features.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    L.shim_recommend_by_index_in_genres.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.shim_recommend_by_index_in_genres.restype = ctypes.c_int64
    csv, out = tmp_path / "dataset.csv", tmp_path / "songs_data.bin"
    _config1_csv(csv)
    assert L.shim_preprocess(str(csv).encode(), str(out).encode()) == 1
    h = L.shim_load(str(out).encode())
    assert h
    try:
        assert L.shim_initialize(h) == 1
        n = 114_000
        feats = np.zeros((n, 12), np.float32)
        gid = np.zeros(n, np.int32)
        g = ctypes.c_int(0)
        for i in range(n):
            L.shim_song_features(h, i, feats[i].ctypes.data, ctypes.byref(g))
            gid[i] = g.value
        for q, wanted in ((0, [gid[0]]), (56_789, [gid[56_789], 100]), (113_999, list(range(114)))):
            gs = np.asarray(wanted, np.int32)
            for topn in (10, 200):
                idx = np.full(topn, -1, np.int32)
                sc = np.zeros(topn, np.float32)
                c = L.shim_recommend_by_index_in_genres(h, q, topn, gs.ctypes.data, gs.size, None, idx.ctypes.data, sc.ctypes.data, topn)
                check((idx[:c].astype(np.int64), sc[:c]), expected(feats, gid, feats[q], q, wanted, topn), f"Recommender row {q}")
    finally:
        L.shim_free(h)
