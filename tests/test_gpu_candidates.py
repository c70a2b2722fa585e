"""CANDIDATE LISTS on the MI355X (csrc/playlist.hip.h, "CANDIDATE LISTS": playlist_gather_rows, the branch of playlist_scan_kernel that
reads only the listed rows), through the _candidates entry points, bit for bit against tests/candidates_oracle.py (the existing CPU
oracles with exclude + the complement of the list): ids, score and distance bits, counts and padding, no tolerances, never against the
code under test.  List sizes at one thread, one workgroup's thread edge, its iteration edge, several workgroups that compact and
exchange thresholds, and every row; on a handle without a replica and on one with it (the gather never consults it), on a lane, and
through a two-shard node handle (row_base != 0)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import distance_oracle, playlist_labels_oracle, prior_oracle
from tests.candidates_oracle import CHUNKS, distinct_in, edge_sizes, gone, request_call
from tests.playlist_labels_oracle import uniform_labels
from tests.rowset_oracle import EXCLUDE, ONLY, prefix
from tests.scaled_oracle import GENERAL, cosine_expected, cosine_scores, distance_expected, distance_m

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
TOPNS = (1, 10, 100, 1024)
METRICS = ("cosine", "euclidean")
FN = {"cosine": "mi355rec_query_playlist_request_candidates", "euclidean": "mi355rec_query_distance_request_candidates"}
NODE_FN = {"cosine": "mi355rec_sharded_query_playlist_request_candidates", "euclidean": "mi355rec_sharded_query_distance_request_candidates"}
ONES = np.ones(12, np.float32)
FOREIGN = np.asarray([2 ** 32 - 1, 70_000, 2 ** 31], np.int64)   # ids of no row of these catalogues: they match nothing
TIES = (1000, 1300)                                              # 300 identical rows (n > 40: copies of row 3)
check = distance_oracle.check   # equal ids, bit-equal scores or distances


def _raw(eng, metric, cand, rowset=None, mode=0, **kw):
    from spotify_recommender_amd import capi
    got = request_call(capi, getattr(eng._lib, FN[metric]), eng._h, metric, cand, rowset._ptr() if rowset is not None else None, mode, **kw)
    assert got[0] == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return got


def _call(eng, metric, cand, rowset=None, mode=0, **kw):
    return _raw(eng, metric, cand, rowset, mode, **kw)[1:3]


def _engines(feats):
    """("replica off", engine) then ("replica on", engine), one alive at a time."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


def _counters(eng):
    from spotify_recommender_amd.engine import candidates_counters
    return candidates_counters(eng)


def _values(metric, feats, members, a=ONES, weights=None):
    return distance_m(feats, members, a) if metric == "euclidean" else cosine_scores(feats, members, a, weights)


def _expected(metric, values, feats, out, topn, where=None, labels=None, wanted=None):
    fn = distance_expected if metric == "euclidean" else cosine_expected
    return fn(values, feats, out, topn, where, labels, wanted)


def _feats(n, seed=1900):
    feats = oracle.mt19937_uniform(seed + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]
        feats[n // 2] = feats[3]
    if n > TIES[1]:
        feats[TIES[0]:TIES[1]] = feats[3]
    return feats


def _list_of(n, size, rng):
    """`size` distinct rows of [0, n) with rows 0 and n - 1 (size >= 2) and, where they fit, the block of identical rows; handed over
    shuffled, with duplicates and with ids that are no row of the catalogue."""
    must = [0, n - 1] if size >= 2 and n >= 2 else [n - 1]
    if n > TIES[1] and size >= 2000:
        must += list(range(*TIES))
    must = np.unique(np.asarray(must, np.int64))
    rest = np.setdiff1d(np.arange(n, dtype=np.int64), must)
    ids = np.concatenate([must, rng.choice(rest, size=size - must.size, replace=False)]) if size > must.size else must[:size]
    assert np.unique(ids).size == size
    handed = rng.permutation(np.concatenate([ids, ids[: min(size, 7)], FOREIGN]))
    return ids, handed


@pytest.mark.parametrize("n", [1, 5, 2049, 65_537])
def test_list_sizes(engine_lib, n):
    feats = _feats(n)
    rng = np.random.default_rng(n)
    sizes = edge_sizes(n) + ([5000] if n > 5000 else [])
    lists = {size: _list_of(n, size, rng) for size in sizes}
    lists["ascending"] = (np.arange(0, n, 3, dtype=np.int64),) * 2          # the host's no-sort path
    members = []
    row = int(rng.integers(0, n))
    vecs = rng.random((min(3, n), 12), dtype=np.float32)
    for metric in METRICS:
        members.append((metric, "by row", dict(rows=[row]), [row], _values(metric, feats, feats[[row]])))
        members.append((metric, "by value", dict(members=vecs), [], _values(metric, feats, vecs)))
    wants = {(i, size): _expected(metric, values, feats, gone(n, ids, own), 1024)
             for i, (metric, _, _, own, values) in enumerate(members) for size, (ids, _) in lists.items()}
    results = {}
    for replica, eng in _engines(feats):
        for size, (ids, handed) in lists.items():
            for i, (metric, by, kw, own, _) in enumerate(members):
                want = wants[(i, size)]
                assert want[0].size == min(1024, ids.size - len(set(own) & set(ids.tolist()))) or metric == "euclidean"
                topns = (10,) if size == 5000 else TOPNS            # (5 000 rows, top-10: every workgroup compacts at 256 keys)
                for topn in topns:
                    before = _counters(eng)
                    got = _call(eng, metric, handed, topn=topn, **kw)
                    after = _counters(eng)
                    check(got, prefix(want, topn), f"n={n} [{replica}] {metric} {by} list of {size} top-{topn}")
                    launched = n - len(own) > 0                      # (n = 1 by row: the member is the catalogue, nothing is launched)
                    assert after["requests"] - before["requests"] == launched, (size, by)
                    assert after["rows_gathered"] - before["rows_gathered"] == (ids.size if launched else 0), (size, by)
                    results.setdefault((i, size, topn), []).append(got)
    for key, (off, on) in results.items():
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [2049, 65_537])
def test_request_kinds(engine_lib, n):
    """One case per kind of request over a list of several workgroups: K = 1 and K = 32 by row and by value, signed weights, filter,
    label set, prior, diversified, capped, distance, scales with either metric, list + seen set, list + only set."""
    from spotify_recommender_amd import capi
    feats = _feats(n, 1300)
    rng = np.random.default_rng([2, n])
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    groups = rng.integers(-1, 40, size=n).astype(np.int32)
    priors = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    ids, handed = _list_of(n, min(5000, n - 40), rng)
    S = rng.permutation(n)[: n // 2].astype(np.int64)
    rows32 = [int(r) for r in rng.choice(ids, size=32, replace=False)]        # members may be listed: never returned
    vecs32 = rng.random((32, 12), dtype=np.float32)
    vecs = vecs32[:3]
    signed = (rng.random(3, dtype=np.float32) + np.float32(0.1)) * np.asarray([1, -1, 1], np.float32)
    ex = [n - 1, 0, 0, 7]
    out, out_ex = gone(n, ids), gone(n, ids, ex)
    sc = cosine_scores(feats, vecs, ONES)
    want = {
        "K=1 by row": cosine_expected(cosine_scores(feats, feats[rows32[:1]], ONES), feats, gone(n, ids, rows32[:1]), 100),
        "K=1 by value": cosine_expected(cosine_scores(feats, vecs[:1], ONES), feats, out, 100),
        "K=32 by row": cosine_expected(cosine_scores(feats, feats[rows32], ONES), feats, gone(n, ids, rows32), 100),
        "K=32 by value": cosine_expected(cosine_scores(feats, vecs32, ONES), feats, out, 100),
        "weights": cosine_expected(cosine_scores(feats, vecs, ONES, signed), feats, out_ex, 100),
        "filter": cosine_expected(sc, feats, out_ex, 100, WHERE),
        "labels": cosine_expected(sc, feats, out_ex, 100, None, lab, WANTED),
        "prior": prior_oracle.expected_prior(sc, priors, -0.5, feats, None, None, out_ex, 100),
        "distance": distance_expected(distance_m(feats, vecs, ONES), feats, out_ex, 100, WHERE, lab, WANTED),
        "distance K=32 by row": distance_expected(distance_m(feats, feats[rows32], ONES), feats, gone(n, ids, rows32), 100),
        "scaled cosine": cosine_expected(cosine_scores(feats, vecs, GENERAL), feats, out_ex, 100),
        "scaled distance": distance_expected(distance_m(feats, vecs, GENERAL), feats, out_ex, 100),
        "list + seen": cosine_expected(sc, feats, gone(n, ids, ex, S, EXCLUDE), 100),
        "list + only": cosine_expected(sc, feats, gone(n, ids, ex, S, ONLY), 100),
        "distance, list + seen": distance_expected(distance_m(feats, vecs, ONES), feats, gone(n, ids, ex, S, EXCLUDE), 100),
    }
    pools = {pool: playlist_labels_oracle.expected_scored(sc, feats, None, None, out_ex, pool) for pool in (40, 1024)}
    results = {}
    for replica, eng in _engines(feats):
        eng.set_labels(lab)
        eng.set_groups(groups)
        eng.set_priors(priors)
        fn = getattr(eng._lib, FN["cosine"])
        with eng.row_set(S) as s:
            got = {
                "K=1 by row": _call(eng, "cosine", handed, rows=rows32[:1], topn=100),
                "K=1 by value": _call(eng, "cosine", handed, members=vecs[:1], topn=100),
                "K=32 by row": _call(eng, "cosine", handed, rows=rows32, topn=100),
                "K=32 by value": _call(eng, "cosine", handed, members=vecs32, topn=100),
                "weights": _call(eng, "cosine", handed, members=vecs, weights=signed, exclude=ex, topn=100),
                "filter": _call(eng, "cosine", handed, members=vecs, exclude=ex, where=WHERE, topn=100),
                "labels": _call(eng, "cosine", handed, members=vecs, exclude=ex, labels=WANTED, topn=100),
                "prior": _call(eng, "cosine", handed, members=vecs, exclude=ex, topn=100, prior_weight=-0.5),
                "distance": _call(eng, "euclidean", handed, members=vecs, exclude=ex, where=WHERE, labels=WANTED, topn=100),
                "distance K=32 by row": _call(eng, "euclidean", handed, rows=rows32, topn=100),
                "scaled cosine": _call(eng, "cosine", handed, members=vecs, exclude=ex, scales=GENERAL, topn=100),
                "scaled distance": _call(eng, "euclidean", handed, members=vecs, exclude=ex, scales=GENERAL, topn=100),
                "list + seen": _call(eng, "cosine", handed, s, EXCLUDE, members=vecs, exclude=ex, topn=100),
                "list + only": _call(eng, "cosine", handed, s, ONLY, members=vecs, exclude=ex, topn=100),
                "distance, list + seen": _call(eng, "euclidean", handed, s, EXCLUDE, members=vecs, exclude=ex, topn=100),
            }
            for kind, g in got.items():
                check(g, want[kind], f"n={n} [{replica}] {kind}")
                results.setdefault(kind, []).append(g)
            for topn, pool in ((10, 40), (100, 1024)):
                rc, gi, gs, gm, _ = request_call(capi, fn, eng._h, "cosine", handed, members=vecs, exclude=ex, topn=topn, lam=0.6, pool=pool)
                assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                wi, ws, wm = playlist_labels_oracle.expected_diverse(pools[pool], feats, 0.6, topn)
                check((gi, gs), (wi, ws), f"n={n} [{replica}] diverse top-{topn} of {pool}")
                assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32))
                rc, gi, gs, gm, p_rows = request_call(capi, fn, eng._h, "cosine", handed, members=vecs, exclude=ex, topn=topn, lam=0.6,
                                                      pool=pool, max_per_group=2)
                assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                wi, ws, wm = playlist_labels_oracle.expected_diverse(pools[pool], feats, 0.6, topn, groups, 2)
                check((gi, gs), (wi, ws), f"n={n} [{replica}] capped top-{topn} of {pool}")
                assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)) and p_rows == pools[pool][0].size
    for kind, (off, on) in results.items():
        check(on, off, f"n={n} {kind}: replica on against off")


def test_padding_empty_results_and_refusals(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    n = 2049
    feats = _feats(n)
    vecs = feats[:2].copy()
    with CosineEngine(feats) as eng:
        L = eng._lib
        for metric in METRICS:
            fn = getattr(L, FN[metric])
            # topn above the admissible count: count and padding as they leave the library
            q = (capi.DistanceQuery if metric == "euclidean" else capi.PlaylistQuery)()
            q.size = ctypes.sizeof(q)
            q.members, q.k, q.topn = vecs.ctypes.data_as(ctypes.c_void_p), 2, 10
            idx, score, count = np.full(10, 99, np.int64), np.full(10, 9.0, np.float32), ctypes.c_int(77)
            pi, ps = idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p)
            res = capi.DistanceResult(pi, ps, ctypes.pointer(count)) if metric == "euclidean" else \
                capi.PlaylistResult(pi, ps, None, ctypes.pointer(count), None)
            cand = np.asarray([2000, 7, 7, 100, 2 ** 32 - 1], np.int64)
            assert fn(eng._h, ctypes.byref(q), None, cand.ctypes.data_as(ctypes.c_void_p), 5, ctypes.byref(res)) == capi.OK
            assert count.value == 3 and sorted(idx[:3].tolist()) == [7, 100, 2000]
            assert idx[3:].tolist() == [-1] * 7 and score[3:].tolist() == [0.0] * 7
            # an empty list and a list of no row of the handle: count 0, nothing is launched; every candidate a member or excluded: count 0
            for what, c, kw in (("empty", [], dict(members=vecs)), ("foreign", FOREIGN, dict(members=vecs)),
                                ("members", [5, 9, 5], dict(rows=[9, 5])), ("excluded", [5, 9], dict(members=vecs, exclude=[5, 9, 11]))):
                before, b_exact = _counters(eng), eng.playlist_counters()
                got = _call(eng, metric, c, topn=10, **kw)
                assert got[0].size == 0, what
                if what in ("empty", "foreign"):              # (members and excluded ids are looked up by the kernel: those launch)
                    assert _counters(eng) == before and eng.playlist_counters()["rows_exact"] == b_exact["rows_exact"], what
            for c, more, msg in (([3, -1], {}, "candidate list: id -1 out of [0, 4294967296)"),
                                 ([2 ** 32], {}, "candidate list: id 4294967296 out of [0, 4294967296)"),
                                 ([1], dict(n_candidates=-1), "candidate list: n_candidates must not be negative, got -1"),
                                 ([1, 2], dict(null_list=True), "candidate list: null list with n_candidates 2"),
                                 ([1], dict(n_candidates=capi.MAX_CANDIDATES + 1),
                                  "candidate list: n_candidates 1048577 above MI355REC_MAX_CANDIDATES (1048576)"),
                                 ([3, -1], dict(ext_size=32), "request ext of size 32: not the end of a field of the 24 bytes this library reads")):
                rc = request_call(capi, fn, eng._h, metric, c, members=vecs, topn=5, **more)[0]
                assert rc == capi.ERR_INVALID_ARG and L.mi355rec_last_error(eng._h).decode() == msg, (metric, msg)


def test_counters_and_requests_without_a_list(engine_lib):
    """The gather's counters rise by 1 and by the distinct in-shard entries; rows_exact rises by exactly the rows the gather admitted
    to the chains, with the replica on as well; a request without a list leaves the gather's counters alone and answers as before."""
    from spotify_recommender_amd.engine import with_candidates
    n = 65_537
    feats = _feats(n, 60)
    rng = np.random.default_rng(6)
    vecs = rng.random((3, 12), dtype=np.float32)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    ids, handed = _list_of(n, 3000, rng)
    S = rng.permutation(n)[: n // 2].astype(np.int64)
    sc = cosine_scores(feats, vecs, ONES)
    for replica, eng in _engines(feats):
        eng.set_labels(lab)
        plain = eng.query_mean_topn(vecs, 50)
        check(plain, cosine_expected(sc, feats, [], 50), f"[{replica}] the plain request")
        with eng.row_set(S) as s:
            admitted = {"list": ids.size, "list + seen": np.setdiff1d(ids, S).size, "list + only": np.intersect1d(ids, S).size,
                        "list + labels": int(np.isin(lab[ids], WANTED).sum()), "list + filter": ids.size}
            calls = {"list": dict(), "list + seen": dict(rowset=s, mode=EXCLUDE), "list + only": dict(rowset=s, mode=ONLY),
                     "list + labels": dict(labels=WANTED), "list + filter": dict(where=WHERE)}
            for what, kw in calls.items():
                for metric in METRICS:
                    c0, e0 = _counters(eng), eng.playlist_counters()
                    _call(eng, metric, handed, members=vecs, topn=10, **kw)
                    c1, e1 = _counters(eng), eng.playlist_counters()
                    assert (c1["requests"] - c0["requests"], c1["rows_gathered"] - c0["rows_gathered"]) == (1, ids.size), what
                    assert e1["rows_exact"] - e0["rows_exact"] == admitted[what], (replica, what, metric)
                    assert e1["queries"] - e0["queries"] == 1
        c0 = _counters(eng)
        check(eng.query_mean_topn(vecs, 50), plain, f"[{replica}] the plain request after the lists")
        check(eng.query_mean_topn(vecs, 50, only=ids), cosine_expected(sc, feats, gone(n, ids), 50), f"[{replica}] only= keeps its route")
        assert _counters(eng) == c0
        check(with_candidates(eng, handed).query_mean_topn(vecs, 50), eng.query_mean_topn(vecs, 50, only=ids), f"[{replica}] the Python form")
        assert _counters(eng)["requests"] == c0["requests"] + 1


def test_a_lane(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import with_candidates
    n = 65_537
    feats = _feats(n, 40)
    rng = np.random.default_rng(12)
    vecs = rng.random((2, 12), dtype=np.float32)
    ids, handed = _list_of(n, max(CHUNKS) * 2 + 1, rng)
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        lane = eng.lane()
        try:
            for metric in METRICS:
                want = _expected(metric, _values(metric, feats, vecs), feats, gone(n, ids), 100)
                check(_call(lane, metric, handed, members=vecs, topn=100), want, f"{metric} on a lane")
                check(_call(eng, metric, handed, members=vecs, topn=100), want, f"{metric} on its parent")
            assert _counters(lane)["requests"] == 2 and _counters(eng)["requests"] == 2      # each handle counts its own
            check(with_candidates(lane, handed).query_nearest(vecs, 20), with_candidates(eng, ids).query_nearest(vecs, 20), "the Python form")
        finally:
            lane.close()


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handle(engine_lib, placement):
    """Two shards on one device: the second has row_base 5004; each gets the ids of its range, a shard with none launches nothing."""
    import torch  # noqa: F401
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine, with_candidates
    n = 10_007
    feats = _feats(n, 10)
    feats[n // 2 - 2:n // 2 + 2] = feats[17]                      # ties across the two shards
    rng = np.random.default_rng(10)
    vecs = rng.random((3, 12), dtype=np.float32)
    rows = [17, 5003, 5004]
    place = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    lists = {"both shards": rng.permutation(np.concatenate([rng.choice(n, size=3000, replace=False), np.arange(5000, 5008), [0, n - 1]])),
             "second shard only": np.arange(n - 1, 5003, -1, dtype=np.int64), "first shard only": np.asarray([5003, 0, 17, 5003], np.int64),
             "every row": np.arange(n, dtype=np.int64)}
    S = rng.permutation(n)[: n // 2].astype(np.int64)
    with NodeEngine(feats, devices=[0, 0], placement=place) as node, node.row_set(S) as s:
        if placement == "sharded":
            assert node.info()["shard_rows"] == [5004, 5003]
        for lname, ids in lists.items():
            for metric in METRICS:
                for kw, own in ((dict(rows=rows, exclude=[1, 9000]), rows), (dict(members=vecs), [])):
                    mem = feats[rows] if "rows" in kw else vecs
                    values = _values(metric, feats, mem)
                    for what, rowset, mode in (("", None, 0), (" + seen", s, EXCLUDE), (" + only", s, ONLY)):
                        got = request_call(capi, getattr(node._lib, NODE_FN[metric]), node._h, metric, ids, rowset._ptr() if rowset else None, mode,
                                           topn=100, **kw)
                        assert got[0] == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                        out = gone(n, ids, list(kw.get("exclude", [])) + own, S if rowset else None, mode)
                        check(got[1:3], _expected(metric, values, feats, out, 100), f"{placement} {lname}{what} {metric}")
            got = request_call(capi, getattr(node._lib, NODE_FN["cosine"]), node._h, "cosine", ids, members=vecs, topn=10, lam=0.6, pool=40)
            assert got[0] == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
            pool_rows = playlist_labels_oracle.expected_scored(cosine_scores(feats, vecs, ONES), feats, None, None, gone(n, ids), 40)
            wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, 10)
            check(got[1:3], (wi, ws), f"{placement} {lname} diverse")
            assert np.array_equal(got[3].view(np.uint32), wm.view(np.uint32))
        rc = request_call(capi, getattr(node._lib, NODE_FN["cosine"]), node._h, "cosine", [3, n], members=vecs, topn=5)[0]
        assert rc == capi.ERR_INVALID_ARG
        assert node._lib.mi355rec_sharded_last_error(node._h).decode() == f"candidate list: id {n} out of [0, {n})"
        ids = lists["both shards"]
        check(with_candidates(node, ids).query_playlist_topn([3, 4], 20, seen=S),
              cosine_expected(cosine_scores(feats, feats[[3, 4]], ONES), feats, gone(n, ids, [3, 4], S, EXCLUDE), 20), "the Python form")
    assert distinct_in(lists["first shard only"], 0, 5004) == 3
