"""CANDIDATE SCORES on the MI355X (csrc/playlist.hip.h, "CANDIDATE SCORES": the score mode of playlist_gather_rows, which stores every
listed row's key and selects nothing), through the mi355rec_score_*_request_candidates entry points, bit for bit against
tests/candidate_scores_oracle.py (the existing CPU oracles' value of every listed row, or the quiet NaN with flag 0): values as uint32
bits, flags exactly, no tolerances, never against the code under test.  The catalogues, list sizes and list shapes are those of
tests/test_gpu_candidates.py."""
import ctypes

import numpy as np
import pytest

from tests import distance_oracle, playlist_labels_oracle, prior_oracle, rowset_oracle
from tests.candidate_scores_oracle import QUIET_NAN, check, expected, score_call
from tests.candidates_oracle import distinct_in, edge_sizes, request_call
from tests.playlist_labels_oracle import uniform_labels
from tests.rowset_oracle import EXCLUDE, ONLY
from tests.scaled_oracle import GENERAL, ONES, cosine_scores, distance_m
from tests.test_gpu_candidates import FN as TOPN_FN
from tests.test_gpu_candidates import FOREIGN, METRICS, WANTED, WHERE, _counters, _engines, _feats, _list_of

pytestmark = pytest.mark.gpu

FN = {"cosine": "mi355rec_score_playlist_request_candidates", "euclidean": "mi355rec_score_distance_request_candidates"}
NODE_FN = {"cosine": "mi355rec_sharded_score_playlist_request_candidates", "euclidean": "mi355rec_sharded_score_distance_request_candidates"}


def _score(eng, metric, cand, rowset=None, mode=0, **kw):
    from spotify_recommender_amd import capi
    rc, values, flags = score_call(capi, getattr(eng._lib, FN[metric]), eng._h, metric, cand, rowset._ptr() if rowset is not None else None,
                                   mode, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return values, flags


def _values(metric, feats, members, a=ONES, weights=None):
    return distance_m(feats, members, a) if metric == "euclidean" else cosine_scores(feats, members, a, weights)


@pytest.mark.parametrize("n", [1, 5, 2049, 4099])
def test_list_sizes(engine_lib, n):
    feats = _feats(n)
    rng = np.random.default_rng(n)
    lists = {size: _list_of(n, size, rng)[1] for size in edge_sizes(n)}
    lists["ascending"] = np.arange(0, n, 3, dtype=np.int64)                 # the host's no-sort path
    row = int(rng.integers(0, n))
    vecs = rng.random((3, 12), dtype=np.float32)
    members = []
    for metric in METRICS:
        members.append((metric, "by row", dict(rows=[row]), [row], _values(metric, feats, feats[[row]])))
        members.append((metric, "by value", dict(members=vecs), [], _values(metric, feats, vecs)))
    wants = {(i, size): expected(n, handed, values, own, metric == "euclidean")
             for i, (metric, _, _, own, values) in enumerate(members) for size, handed in lists.items()}
    results = {}
    for replica, eng in _engines(feats):
        for size, handed in lists.items():
            for i, (metric, by, kw, _, _) in enumerate(members):
                got = _score(eng, metric, handed, topn=1, **kw)
                check(got, wants[(i, size)], f"n={n} [{replica}] {metric} {by} list of {size}")
                results.setdefault((i, size), []).append(got)
    for key, (off, on) in results.items():
        assert np.array_equal(off[0].view(np.uint32), on[0].view(np.uint32)) and np.array_equal(off[1], on[1]), f"n={n} {key}: replica on against off"


def test_options(engine_lib):
    n = 4099
    feats = _feats(n, 1300)
    rng = np.random.default_rng([21, n])
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    priors = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    handed = _list_of(n, 2049, rng)[1]
    S = rng.permutation(n)[: n // 2].astype(np.int64)
    rows32 = [int(r) for r in rng.choice(handed[handed < n], size=32, replace=False)]
    vecs = rng.random((3, 12), dtype=np.float32)
    signed = ((rng.random(32, dtype=np.float32) + np.float32(0.1)) * np.where(np.arange(32) % 3 == 1, -1, 1)).astype(np.float32)
    ex = [n - 1, 0, 0, 7]
    sc = cosine_scores(feats, vecs, ONES)
    bad = playlist_labels_oracle.inadmissible(feats, lab, WANTED, WHERE)
    want = {
        "weights K=32 by row": expected(n, handed, cosine_scores(feats, feats[rows32], ONES, signed), rows32),
        "prior +4": expected(n, handed, prior_oracle.blended(sc, priors, 4.0), ex),
        "prior -4": expected(n, handed, prior_oracle.blended(sc, priors, -4.0), ex),
        "scaled cosine": expected(n, handed, cosine_scores(feats, vecs, GENERAL), ex),
        "scaled distance": expected(n, handed, distance_m(feats, vecs, GENERAL), ex, True),
        "exclude + filter + labels": expected(n, handed, sc, np.concatenate([ex, bad])),
        "distance: exclude + filter + labels": expected(n, handed, distance_m(feats, vecs, ONES), np.concatenate([ex, bad]), True),
        "seen": expected(n, handed, sc, rowset_oracle.excluded(n, S, EXCLUDE, ex)),
        "only": expected(n, handed, sc, rowset_oracle.excluded(n, S, ONLY, ex)),
        "distance, seen": expected(n, handed, distance_m(feats, vecs, ONES), rowset_oracle.excluded(n, S, EXCLUDE, ex), True),
    }
    assert not want["weights K=32 by row"][1][np.isin(handed, rows32)].any()          # members by row come out inadmissible
    results = {}
    for replica, eng in _engines(feats):
        eng.set_labels(lab)
        eng.set_priors(priors)
        with eng.row_set(S) as s:
            got = {
                "weights K=32 by row": _score(eng, "cosine", handed, rows=rows32, weights=signed, topn=5),
                "prior +4": _score(eng, "cosine", handed, members=vecs, exclude=ex, topn=5, prior_weight=4.0),
                "prior -4": _score(eng, "cosine", handed, members=vecs, exclude=ex, topn=5, prior_weight=-4.0),
                "scaled cosine": _score(eng, "cosine", handed, members=vecs, exclude=ex, scales=GENERAL, topn=5),
                "scaled distance": _score(eng, "euclidean", handed, members=vecs, exclude=ex, scales=GENERAL, topn=5),
                "exclude + filter + labels": _score(eng, "cosine", handed, members=vecs, exclude=ex, where=WHERE, labels=WANTED, topn=5),
                "distance: exclude + filter + labels": _score(eng, "euclidean", handed, members=vecs, exclude=ex, where=WHERE, labels=WANTED, topn=5),
                "seen": _score(eng, "cosine", handed, s, EXCLUDE, members=vecs, exclude=ex, topn=5),
                "only": _score(eng, "cosine", handed, s, ONLY, members=vecs, exclude=ex, topn=5),
                "distance, seen": _score(eng, "euclidean", handed, s, EXCLUDE, members=vecs, exclude=ex, topn=5),
            }
        for kind, g in got.items():
            check(g, want[kind], f"[{replica}] {kind}")
            results.setdefault(kind, []).append(g)
    for kind, (off, on) in results.items():
        assert np.array_equal(off[0].view(np.uint32), on[0].view(np.uint32)) and np.array_equal(off[1], on[1]), kind


def test_hostile_catalogue(engine_lib):
    """Rows with NaN, +-inf and 1e30: m is not finite there: NaN and flag 0, for members by value and by row."""
    n = 2049
    feats = distance_oracle.hostile_catalogue(n)
    handed = np.random.default_rng(3).permutation(np.concatenate([np.arange(n, dtype=np.int64), FOREIGN, [2, 3, 4, 7]]))
    vecs = feats[[0, 10]].copy()
    wants = {"by value": expected(n, handed, distance_oracle.mean_sqdist(feats, vecs), [], True),
             "by row": expected(n, handed, distance_oracle.mean_sqdist(feats, feats[[10, 11]]), [10, 11], True)}
    assert not wants["by value"][1][np.isin(handed, [2, 3, 4, 7])].any() and wants["by value"][1].sum() > n - 10
    for replica, eng in _engines(feats):
        check(_score(eng, "euclidean", handed, members=vecs, topn=3), wants["by value"], f"[{replica}] by value")
        check(_score(eng, "euclidean", handed, rows=[10, 11], topn=3), wants["by row"], f"[{replica}] by row")


def test_consistency_with_the_topn_call(engine_lib):
    from spotify_recommender_amd import capi
    n = 4099
    feats = _feats(n, 77)
    rng = np.random.default_rng(77)
    vecs = rng.random((3, 12), dtype=np.float32)
    ids, handed = _list_of(n, 3000, rng)
    ex = [0, 9, n - 1]
    for replica, eng in _engines(feats):
        for metric in METRICS:
            def topn_call():
                got = request_call(capi, getattr(eng._lib, TOPN_FN[metric]), eng._h, metric, handed, members=vecs, exclude=ex, topn=1024)
                assert got[0] == capi.OK
                return got[1], got[2]
            before = topn_call()
            values, flags = _score(eng, metric, handed, members=vecs, exclude=ex, topn=1024)
            after = topn_call()
            distance_oracle.check(after, before, f"[{replica}] {metric}: the top-N call after the scoring call")
            where = {int(g): i for i, g in enumerate(handed.tolist())}
            at = np.asarray([where[int(g)] for g in before[0]], np.int64)
            assert flags[at].all() and np.array_equal(values[at].view(np.uint32), before[1].view(np.uint32)), (replica, metric)
            adm_ids, first = np.unique(handed[flags.astype(bool)], return_index=True)
            adm_val = values[flags.astype(bool)][first]
            order = np.lexsort((adm_ids, adm_val if metric == "euclidean" else -adm_val))[:1024]
            if metric == "cosine":
                assert adm_ids[order].tolist() == before[0].tolist(), replica
            else:   # (the call ranks by m, the values are sqrtf(m): two m may share a root, so ids are compared where the root is unique)
                assert np.array_equal(adm_val[order].view(np.uint32), before[1].view(np.uint32)), replica
                _, inverse, counts = np.unique(adm_val, return_inverse=True, return_counts=True)
                single = counts[inverse][order] == 1
                assert single.sum() > 600 and adm_ids[order][single].tolist() == before[0][single].tolist(), replica


def test_grid_stride(engine_lib):
    """A list of every row of a catalogue with more rows than the gather launch's grid (at most CUs x 2 = 512 workgroups,
    engine_playlist.hip.h: grid_cap) times the 1024 entries of a workgroup's iteration, and a tail that is no multiple of 1024: workgroups
    take a second chunk, so the store index runs past one chunk per workgroup."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    n = 512 * 1024 + 1024 + 37
    feats = np.random.default_rng(2100).random((n, 12), dtype=np.float32)
    vec = np.random.default_rng(2101).random((1, 12), dtype=np.float32)
    handed = np.arange(n, dtype=np.int64)
    want = expected(n, handed, playlist_labels_oracle.scores_of(feats, vec), [5, n - 1])
    with CosineEngine(feats) as eng:
        check(_score(eng, "cosine", handed, members=vec, exclude=[5, n - 1], topn=1), want, "every row of 525 349")


def test_a_lane(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    n = 4099
    feats = _feats(n, 40)
    rng = np.random.default_rng(12)
    vecs = rng.random((2, 12), dtype=np.float32)
    handed = _list_of(n, 2049, rng)[1]
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        lane = eng.lane()
        try:
            for metric in METRICS:
                want = expected(n, handed, _values(metric, feats, vecs), [], metric == "euclidean")
                check(_score(lane, metric, handed, members=vecs, topn=1), want, f"{metric} on a lane")
                check(_score(eng, metric, handed, members=vecs, topn=1), want, f"{metric} on its parent")
            assert _counters(lane)["requests"] == 2 and _counters(eng)["requests"] == 2      # each handle counts its own
        finally:
            lane.close()


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handle(engine_lib, placement):
    """Two shards on one device, split unevenly: the second has row_base 2050; each scores the ids of its range, a shard with none
    launches nothing."""
    import torch  # noqa: F401
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine, candidate_scores
    n = 4099
    feats = _feats(n, 10)
    rng = np.random.default_rng(10)
    vecs = rng.random((3, 12), dtype=np.float32)
    rows = [17, 2049, 2050]
    place = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    lists = {"both shards": rng.permutation(np.concatenate([rng.choice(n, size=1500, replace=False), np.arange(2046, 2054), [0, n - 1, 0]])),
             "second shard only": np.arange(n - 1, 2049, -1, dtype=np.int64), "first shard only": np.asarray([2049, 0, 17, 2049], np.int64)}
    S = rng.permutation(n)[: n // 2].astype(np.int64)
    with NodeEngine(feats, devices=[0, 0], placement=place) as node, node.row_set(S) as s:
        if placement == "sharded":
            assert node.info()["shard_rows"] == [2050, 2049]
        for lname, ids in lists.items():
            for metric in METRICS:
                for kw, own in ((dict(rows=rows, exclude=[1, 3000]), rows), (dict(members=vecs), [])):
                    values = _values(metric, feats, feats[rows] if "rows" in kw else vecs)
                    for what, rowset, mode in (("", None, 0), (" + seen", s, EXCLUDE), (" + only", s, ONLY)):
                        rc, gv, gf = score_call(capi, getattr(node._lib, NODE_FN[metric]), node._h, metric, ids, rowset._ptr() if rowset else None,
                                                mode, topn=1, **kw)
                        assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                        gone = list(kw.get("exclude", [])) + own + (rowset_oracle.excluded(n, S, mode).tolist() if rowset else [])
                        check((gv, gf), expected(n, ids, values, gone, metric == "euclidean"), f"{placement} {lname}{what} {metric}")
        rc = score_call(capi, getattr(node._lib, NODE_FN["cosine"]), node._h, "cosine", [3, n], members=vecs, topn=5)[0]
        assert rc == capi.ERR_INVALID_ARG
        assert node._lib.mi355rec_sharded_last_error(node._h).decode() == f"candidate list: id {n} out of [0, {n})"
        ids = lists["both shards"]
        check(candidate_scores(node, ids, rows=[3, 4], seen=S),
              expected(n, ids, cosine_scores(feats, feats[[3, 4]], ONES), [3, 4] + S.tolist()), "the Python form")
    assert distinct_in(lists["first shard only"], 0, 2050) == 3


def test_arguments_and_counters(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import candidate_scores
    n = 2049
    feats = _feats(n)
    vecs = feats[:2].copy()
    rng = np.random.default_rng(5)
    ids, handed = _list_of(n, 1500, rng)
    with CosineEngine(feats) as eng:
        L = eng._lib
        for metric in METRICS:
            fn = getattr(L, FN[metric])
            for c, more, msg in (([3, -1], {}, "candidate list: id -1 out of [0, 4294967296)"),
                                 ([2 ** 32], {}, "candidate list: id 4294967296 out of [0, 4294967296)"),
                                 ([1], dict(n_candidates=-1), "candidate list: n_candidates must not be negative, got -1"),
                                 ([1, 2], dict(null_list=True), "candidate list: null list with n_candidates 2"),
                                 ([1], dict(n_candidates=capi.MAX_CANDIDATES + 1),
                                  "candidate list: n_candidates 1048577 above MI355REC_MAX_CANDIDATES (1048576)"),
                                 ([3, -1], dict(ext_size=32), "request ext of size 32: not the end of a field of the 24 bytes this library reads"),
                                 ([3], dict(topn=0), "topn 0 out of [1, 1024] (a playlist query has one round)"),
                                 ([3, 4], dict(null_value=True), "candidate scores: null out_value with n_candidates 2")):
                kw = dict(members=vecs, topn=5)
                kw.update(more)
                rc = score_call(capi, fn, eng._h, metric, c, **kw)[0]
                assert rc == capi.ERR_INVALID_ARG and L.mi355rec_last_error(eng._h).decode() == msg, (metric, msg)
            # n_candidates == 0: OK, nothing written, nothing launched (NULL outputs are fine then)
            before, b_exact = _counters(eng), eng.playlist_counters()
            rc, gv, gf = score_call(capi, fn, eng._h, metric, [], members=vecs, topn=5, null_value=True, null_flags=True)
            assert rc == capi.OK and _counters(eng) == before and eng.playlist_counters() == b_exact
            # a list of no row of the handle: every entry NaN / 0, nothing launched
            rc, gv, gf = score_call(capi, fn, eng._h, metric, FOREIGN, members=vecs, topn=5)
            assert rc == capi.OK and gv.view(np.uint32).tolist() == [QUIET_NAN] * 3 and gf.tolist() == [0] * 3 and _counters(eng) == before
            # NULL out_admissible: the values alone
            want = expected(n, handed, _values(metric, feats, vecs), [], metric == "euclidean")
            rc, gv, gf = score_call(capi, fn, eng._h, metric, handed, members=vecs, topn=5, null_flags=True)
            assert rc == capi.OK and np.array_equal(gv.view(np.uint32), want[0]) and gf.tolist() == [7] * handed.size
            # the counters rise as the _candidates call's do on the same list
            c0, e0 = _counters(eng), eng.playlist_counters()
            assert request_call(capi, getattr(L, TOPN_FN[metric]), eng._h, metric, handed, members=vecs, where=WHERE, topn=5)[0] == capi.OK
            c1, e1 = _counters(eng), eng.playlist_counters()
            assert score_call(capi, fn, eng._h, metric, handed, members=vecs, where=WHERE, topn=5)[0] == capi.OK
            c2, e2 = _counters(eng), eng.playlist_counters()
            assert {k: c2[k] - c1[k] for k in c1} == {k: c1[k] - c0[k] for k in c0} == {"requests": 1, "rows_gathered": ids.size}
            assert {k: e2[k] - e1[k] for k in e1} == {k: e1[k] - e0[k] for k in e0}
        fn = getattr(L, FN["cosine"])
        for more, flag in ((dict(lam=0.5, pool=10), "MI355REC_PQ_DIVERSE"), (dict(lam=0.5, pool=10, max_per_group=2), "MI355REC_PQ_CAPPED")):
            rc = score_call(capi, fn, eng._h, "cosine", [3, 4], members=vecs, topn=5, **more)[0]
            assert rc == capi.ERR_INVALID_ARG
            assert L.mi355rec_last_error(eng._h).decode() == f"{flag} in a candidate scores call: a re-ranked order has no per-row value"
        # the Python form, members by row and by value
        check(candidate_scores(eng, handed, rows=[3], exclude=[9]), expected(n, handed, cosine_scores(feats, feats[[3]], ONES), [3, 9]), "rows=")
        check(candidate_scores(eng, handed, queries=vecs, metric="distance", only=ids[:700]),
              expected(n, handed, distance_m(feats, vecs, ONES), rowset_oracle.excluded(n, ids[:700], ONLY), True), "queries=, distance, only=")
