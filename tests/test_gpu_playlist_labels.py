"""PLAYLIST REQUESTS on the MI355X: the playlist family within a LABEL SET (csrc/playlist.hip.h, "LABEL SET": the label test
of playlist_scan_kernel, before the 8-bit dot products, the filter and the chains), bit for bit against the composed oracle
(tests/playlist_labels_oracle.py): ids, score bits and counts, no tolerances.  Sizes around every boundary of the kernel (the
tail quad and the label padding, the 2048-row tile, the 4096-row anchor table, the replica's 65 536 rows) and a 262 144-row
catalogue on which the pre-filter and the anchor bound are live."""
import numpy as np
import pytest

from oracle import oracle
from tests.diverse_oracle import check3
from tests.labels_oracle import check
from tests.playlist_labels_oracle import (contiguous_labels, expected_diverse, expected_scored, request_call, scores_of, uniform_labels)

pytestmark = pytest.mark.gpu

N_BIG = 262_144
N_LABELS = 114
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
SIZES = [1, 3, 4, 5, 2047, 2048, 2049, 4095, 4096, 4097, 65_535, 65_536, 65_537]


@pytest.fixture(scope="module")
def big(engine_lib):
    """(engine, feats, {layout: labels}, member rows, {k: scores of every row}): computed once, never modified."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine
    feats = oracle.mt19937_uniform(2024, N_BIG)
    lay = {"uniform": uniform_labels(N_BIG, N_LABELS, 7), "contiguous": contiguous_labels(N_BIG, N_LABELS)}
    rows = np.random.default_rng(11).choice(N_BIG, size=32, replace=False)
    scores = {k: scores_of(feats, feats[rows[:k]]) for k in (1, 10, 32)}
    with CosineEngine(feats) as eng:
        yield eng, feats, lay, rows, scores


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    feats = oracle.mt19937_uniform(300 + n % 97, n)
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    lab[n - 1] = 2                                        # the last row (the tail quad) is selectable
    full = rng.integers(0, 6, size=n).astype(np.int32)    # no -1 anywhere
    k = min(3, n)
    rows = rng.choice(n, size=k, replace=False)
    vecs = rng.random((k, 12), dtype=np.float32)
    s_rows, s_vecs = scores_of(feats, feats[rows]), scores_of(feats, vecs)
    with CosineEngine(feats) as eng:
        eng.set_labels(full)
        for topn in (1, 10):
            # every label selected, no row unlabelled: the unlabelled call, bit for bit
            check(eng.query_playlist_topn(rows, topn, labels=range(6)), eng.query_playlist_topn(rows, topn), f"n={n} all labels by row")
            check(eng.query_mean_topn(vecs, topn, labels=range(6)), eng.query_mean_topn(vecs, topn), f"n={n} all labels by value")
        eng.set_labels(lab)
        for topn in (1, 10, 1024):
            for wanted in ([2], [0, 2, 5], [5, 5, 1], [9]):   # (9: a label without rows -> count 0)
                what = f"n={n} top-{topn} labels {wanted}"
                got = eng.query_playlist_topn(rows, topn, labels=wanted)
                check(got, expected_scored(s_rows, feats, lab, wanted, rows, topn), what + " by row")
                assert not np.any(lab[got[0]] < 0), what
                check(eng.query_mean_topn(vecs, topn, [n - 1], labels=wanted), expected_scored(s_vecs, feats, lab, wanted, [n - 1], topn),
                      what + " by value, the last row excluded")
                check(eng.query_mean_topn(vecs, topn, where=WHERE, labels=wanted),
                      expected_scored(s_vecs, feats, lab, wanted, [], topn, WHERE), what + " filtered")
        # K = 1 by row is the label route's single query
        for q in {0, n // 2, n - 1}:
            for wanted in ([2], [0, 1, 2, 3, 4, 5]):
                check(eng.query_playlist_topn([q], 10, labels=wanted), eng.query_row_topn_labels(q, wanted, 10), f"n={n} row {q} {wanted}")
        # contiguous labels: whole quads and tiles fail the test
        cont = contiguous_labels(n, 6)
        eng.set_labels(cont)
        for wanted in ([0], [5], [1, 4]):
            check(eng.query_mean_topn(vecs, 10, labels=wanted), expected_scored(s_vecs, feats, cont, wanted, [], 10), f"n={n} contiguous {wanted}")


@pytest.mark.parametrize("layout", ["uniform", "contiguous"])
@pytest.mark.parametrize("k", [1, 10, 32])
def test_262k_matches_the_oracle(big, layout, k):
    eng, feats, lay, rows, scores = big
    lab = lay[layout]
    eng.set_labels(lab)
    members = rows[:k]
    rng = np.random.default_rng(k)
    outside = np.flatnonzero(lab != lab[members[0]])[:3].tolist()
    sets = {"1 label": [int(lab[members[0]]) if lab[members[0]] >= 0 else 3], "3 labels": [5, 60, 113], "all": list(range(N_LABELS)),
            "members outside": [int(l) for l in range(N_LABELS) if l not in set(lab[members].tolist())][:4]}
    for name, wanted in sets.items():
        top = expected_scored(scores[k], feats, lab, wanted, members, 200)[0]
        excl = np.concatenate([top[::2], rng.integers(0, N_BIG, size=200), outside])   # excluded ids inside and outside the selection
        for topn in (10, 1024):
            what = f"{layout} k={k} {name} top-{topn}"
            got = eng.query_playlist_topn(members, topn, labels=wanted)
            check(got, expected_scored(scores[k], feats, lab, wanted, members, topn), what)
            assert not np.any(lab[got[0]] < 0) and not set(got[0].tolist()) & set(members.tolist()), what
            check(eng.query_playlist_topn(members, topn, excl, labels=wanted),
                  expected_scored(scores[k], feats, lab, wanted, list(members) + excl.tolist(), topn), what + " excluded")
            check(eng.query_mean_topn(feats[members], topn, excl, where=WHERE, labels=wanted),
                  expected_scored(scores[k], feats, lab, wanted, excl, topn, WHERE), what + " by value, filtered")
    if k == 1:
        q = int(members[0])
        for wanted in sets.values():
            for topn in (10, 1024):
                check(eng.query_playlist_topn([q], topn, labels=wanted), eng.query_row_topn_labels(q, wanted, topn), f"{layout} row {q} {wanted[:3]}")


def test_few_rows_and_no_rows(big):
    eng, feats, lay, rows, scores = big
    lab = lay["uniform"].copy()
    lab[lab == 7] = 8
    lab[[5, 99_999, N_BIG - 1]] = 7          # three rows of label 7, none of label 200
    eng.set_labels(lab)
    ids, sc = eng.query_playlist_topn(rows[:10], 10, labels=[7])
    assert sorted(ids.tolist()) == [5, 99_999, N_BIG - 1]
    check((ids, sc), expected_scored(scores[10], feats, lab, [7], rows[:10], 10), "three rows")
    # count below topn: request_call checks the padding behind it (idx -1, score and mmr 0), plain and re-ranked
    fn = eng._lib.mi355rec_query_playlist_request
    rc, ids, sc, _, _ = request_call(_capi(), fn, eng._h, rows=rows[:10], labels=[7], topn=10)
    assert rc == 0 and ids.size == 3
    rc, ids, sc, mmr, _ = request_call(_capi(), fn, eng._h, rows=rows[:10], labels=[7], topn=10, lam=0.5, pool=64)
    assert rc == 0 and sorted(ids.tolist()) == [5, 99_999, N_BIG - 1]
    before = eng.playlist_counters()["rows_exact"]
    assert eng.query_playlist_topn(rows[:10], 10, labels=[200, 201])[0].size == 0
    for kw in (dict(), dict(lam=0.5, pool=64)):               # nothing selected: count 0, every slot padded
        rc, ids, sc, mmr, _ = request_call(_capi(), fn, eng._h, rows=rows[:10], labels=[200, 201], topn=10, **kw)
        assert rc == 0 and ids.size == 0
    assert eng.playlist_counters()["rows_exact"] == before      # nothing selected: nothing launched


def _capi():
    from spotify_recommender_amd import capi
    return capi


def test_dislikes_switch_the_prefilter_off(big):
    eng, feats, lay, rows, scores = big
    lab = lay["uniform"]
    eng.set_labels(lab)
    vecs = np.random.default_rng(3).random((4, 12), dtype=np.float32)
    vecs[2:] = vecs[:2]
    w = np.array([1.0, 1.0, -1.0, -1.0], np.float32)            # likes and dislikes cancel: |u| = 0, every selected row takes the chains
    wanted = [1, 50, 51, 52]
    s = scores_of(feats, vecs, w)
    before = eng.playlist_counters()["rows_exact"]
    check(eng.query_mean_topn(vecs, 100, weights=w, labels=wanted), expected_scored(s, feats, lab, wanted, [], 100), "cancelling")
    assert eng.playlist_counters()["rows_exact"] - before == int(np.isin(lab, wanted).sum())   # rejected rows are not counted
    w2 = np.where(np.arange(10) % 3 == 2, -0.5, 1.0).astype(np.float32)
    s2 = scores_of(feats, feats[rows[:10]], w2)
    check(eng.query_playlist_topn(rows[:10], 100, weights=w2, where=WHERE, labels=wanted),
          expected_scored(s2, feats, lab, wanted, rows[:10], 100, WHERE), "dislikes, filtered")


@pytest.mark.parametrize("layout", ["uniform", "contiguous"])
def test_diversified_and_capped_pools_are_admissible_rows(big, layout):
    eng, feats, lay, rows, scores = big
    lab = lay[layout]
    eng.set_labels(lab)
    groups = (np.arange(N_BIG) % 5).astype(np.int32)
    eng.set_groups(groups)
    try:
        members = rows[:10]
        for wanted, pool in (([5, 60, 113], 64), (list(range(N_LABELS)), 256), ([5], 1024)):
            pl = expected_scored(scores[10], feats, lab, wanted, members, pool, WHERE)
            assert set(np.unique(lab[pl[0]]).tolist()) <= set(wanted)
            for lam in (0.5, 1.0):
                what = f"{layout} {wanted[:3]} pool {pool} lambda {lam}"
                got = eng.query_playlist_topn_diverse(members, 10, lam, pool, where=WHERE, return_mmr=True, labels=wanted)
                check3(got, expected_diverse(pl, feats, lam, 10), what)
                got = eng.query_playlist_topn_capped(members, 10, 1, lam, pool, where=WHERE, return_mmr=True, return_pool_rows=True, labels=wanted)
                check3(got[:3], expected_diverse(pl, feats, lam, 10, groups, 1), what + " capped")
                assert got[3] == pl[0].size, what
        tight = {0: (0.0, 0.02)}                                # fewer admissible rows than the pool: P' < pool
        pl = expected_scored(scores[10], feats, lab, [5], members, 1024, tight)
        assert 0 < pl[0].size < 1024
        got = eng.query_playlist_topn_capped(members, 10, 2, 0.7, 1024, where=tight, return_mmr=True, return_pool_rows=True, labels=[5])
        check3(got[:3], expected_diverse(pl, feats, 0.7, 10, groups, 2), "tight")
        assert got[3] == pl[0].size
    finally:
        eng.set_groups(None)


def test_prefilter_stays_live_and_unlabelled_calls_are_unchanged(big):
    eng, feats, lay, rows, scores = big
    eng.set_labels(lay["uniform"])
    members = rows[:10]
    plain = eng.query_playlist_topn(members, 100, [4, 5])
    b0 = eng.playlist_counters()
    eng.query_playlist_topn(members, 100, [4, 5])
    plain_rows = eng.playlist_counters()["rows_exact"] - b0["rows_exact"]
    broad = list(range(100))
    selected = int(np.isin(lay["uniform"], broad).sum())
    b1 = eng.playlist_counters()
    got = eng.query_playlist_topn(members, 100, [4, 5], labels=broad)
    a1 = eng.playlist_counters()
    check(got, expected_scored(scores[10], feats, lay["uniform"], broad, list(members) + [4, 5], 100), "broad")
    assert a1["queries"] == b1["queries"] + 1
    grown = a1["rows_exact"] - b1["rows_exact"]
    print(f"rows_exact: unlabelled {plain_rows}, {len(broad)} labels ({selected} rows selected) {grown}")
    assert 0 < grown < selected
    check(eng.query_playlist_topn(members, 100, [4, 5]), plain, "unlabelled after labelled")


def test_old_entry_points_are_the_request_call(big):
    """The ten single-handle entry points against mi355rec_query_playlist_request with the same fields."""
    eng, feats, lay, rows, scores = big
    capi = _capi()
    fn = eng._lib.mi355rec_query_playlist_request
    eng.set_groups((np.arange(N_BIG) % 3).astype(np.int32))
    try:
        r, v, ex, w = [int(x) for x in rows[:5]], feats[rows[5:9]], [1, 2, 3], [1.0, -0.5, 2.0, 0.25]
        w5 = w + [1.5]
        for by, members, ww, old in (("rows", r, w5, "playlist"), ("members", v, w, "mean")):
            m = {by: members}
            f = getattr(eng, f"query_{old}_topn")
            cases = [(f(members, 20, ex), dict(exclude=ex)), (f(members, 20, ex, where=WHERE), dict(exclude=ex, where=WHERE)),
                     (f(members, 20, ex, where=WHERE, weights=ww), dict(exclude=ex, where=WHERE, weights=ww))]
            for want, kw in cases:
                rc, ids, sc, _, _ = request_call(capi, fn, eng._h, topn=20, **m, **kw)
                assert rc == 0
                check((ids, sc), want, f"{old} {sorted(kw)}")
            want = getattr(eng, f"query_{old}_topn_diverse")(members, 20, 0.4, 100, ex, WHERE, ww, return_mmr=True)
            rc, ids, sc, mmr, _ = request_call(capi, fn, eng._h, topn=20, exclude=ex, where=WHERE, weights=ww, lam=0.4, pool=100, **m)
            assert rc == 0
            check3((ids, sc, mmr), want, f"{old} diverse")
            want = getattr(eng, f"query_{old}_topn_capped")(members, 20, 2, 0.4, 100, ex, WHERE, ww, return_mmr=True, return_pool_rows=True)
            rc, ids, sc, mmr, p = request_call(capi, fn, eng._h, topn=20, exclude=ex, where=WHERE, weights=ww, lam=0.4, pool=100, max_per_group=2, **m)
            assert rc == 0 and p == want[3]
            check3((ids, sc, mmr), want[:3], f"{old} capped")
    finally:
        eng.set_groups(None)


def test_lane_answers_as_its_parent(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    n = 70_001
    feats = oracle.mt19937_uniform(17, n)
    lab = uniform_labels(n, 20, 17)
    rows, wanted = [7, 7_000, 69_999], [0, 3, 19]
    with CosineEngine(feats) as eng:
        eng.set_labels(lab)
        want = eng.query_playlist_topn(rows, 200, [8, 9], where=WHERE, labels=wanted)
        lane = eng.lane()
        try:
            check(lane.query_playlist_topn(rows, 200, [8, 9], where=WHERE, labels=wanted), want, "lane")
        finally:
            lane.close()
        check(want, expected_scored(scores_of(feats, feats[rows]), feats, lab, wanted, rows + [8, 9], 200, WHERE), "oracle")


def test_replacing_and_dropping_the_labels(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    n = 70_001
    feats = oracle.mt19937_uniform(18, n)
    a, b = uniform_labels(n, 20, 1), contiguous_labels(n, 20)
    rows, wanted = [1, 2, 35_000], [4, 5]
    s = scores_of(feats, feats[rows])
    with CosineEngine(feats) as eng:
        with pytest.raises(capi.Mi355Error, match="has no labels"):
            eng.query_playlist_topn(rows, 10, labels=wanted)
        for lab in (a, b, a):
            eng.set_labels(lab)
            check(eng.query_playlist_topn(rows, 50, labels=wanted), expected_scored(s, feats, lab, wanted, rows, 50), "replaced")
        plain = eng.query_playlist_topn(rows, 50)
        eng.set_labels(None)
        with pytest.raises(capi.Mi355Error, match="has no labels") as e:
            eng.query_playlist_topn(rows, 10, labels=wanted)
        assert e.value.code == capi.ERR_INVALID_ARG
        check(eng.query_playlist_topn(rows, 50), plain, "unlabelled after the drop")
        eng.set_labels(a)
        for kw, msg in ((dict(labels=[1024]), "label 1024 out of"), (dict(labels=[-1]), "label -1 out of"), (dict(labels=[]), "n_labels must be positive"),
                        (dict(n_labels=-1), "n_labels must be positive"), (dict(n_labels=2), "null label set")):
            rc = request_call(capi, eng._lib.mi355rec_query_playlist_request, eng._h, rows=rows, topn=10, **kw)[0]
            assert rc == capi.ERR_INVALID_ARG and msg in eng._lib.mi355rec_last_error(eng._h).decode(), (kw, msg)


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(9, n)
    lab = uniform_labels(n, 30, 9)
    groups = (np.arange(n) % 4).astype(np.int32)
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    rng = np.random.default_rng(9)
    with CosineEngine(feats) as single, NodeEngine(feats, devices=[0, 0], placement=pl) as node:
        with pytest.raises(capi.Mi355Error, match="has no labels"):
            node.query_playlist_topn([1, 2], 10, labels=[1])
        for e in (single, node):
            e.set_labels(lab)
            e.set_groups(groups)
        for k in (1, 6, 32):
            rows = rng.choice(n, size=k, replace=False)
            excl = rng.integers(0, n, size=500)
            for wanted in ([3], [0, 7, 29], list(range(30))):
                for topn in (10, 1024):
                    want = single.query_playlist_topn(rows, topn, excl, where=WHERE, labels=wanted)
                    check(node.query_playlist_topn(rows, topn, excl, where=WHERE, labels=wanted), want, f"{placement} by row k={k}")
                    check(node.query_mean_topn(feats[rows], topn, excl, labels=wanted), single.query_mean_topn(feats[rows], topn, excl, labels=wanted),
                          f"{placement} by value k={k}")
                check(want, expected_scored(scores_of(feats, feats[rows]), feats, lab, wanted, list(rows) + excl.tolist(), 1024, WHERE), "oracle")
                kw = dict(where=WHERE, return_mmr=True, return_pool_rows=True, labels=wanted)
                got = node.query_playlist_topn_capped(rows, 10, 1, 0.5, 64, excl, **kw)
                want4 = single.query_playlist_topn_capped(rows, 10, 1, 0.5, 64, excl, **kw)
                check3(got[:3], want4[:3], f"{placement} capped k={k}")
                assert got[3] == want4[3]
