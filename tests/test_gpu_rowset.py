"""ROW SETS on the MI355X (csrc/playlist.hip.h, "ROW SETS": the bit test at the top of playlist_scan_kernel's tile iteration and in
its anchor bound), through the _ext entry points, bit for bit against tests/rowset_oracle.py (the existing oracles with exclude + S,
or exclude + the complement of S): ids, score and distance bits, counts and padding, no tolerances.  Sizes at the quad, the byte (two
quads), the word, the 2048-row tile and its tail, kPlBoundRows, the 4096-row anchor table and 33 workgroups that publish thresholds;
on a handle without a replica (every admitted row takes the chains) and on one with a replica, and the two must agree."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import distance_oracle, playlist_labels_oracle, prior_oracle
from tests.playlist_labels_oracle import uniform_labels
from tests.rowset_oracle import EXCLUDE, MODES, ONLY, excluded, prefix, request_call, shapes
from tests.scaled_oracle import GENERAL, cosine_expected, cosine_scores, distance_expected, distance_m

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 4, 5, 7, 8, 9, 31, 32, 33, 257, 2047, 2048, 2049, 4097, 65_537]
COMPOSED = [257, 4097, 65_537]
TOPNS = (1, 10, 1024)
METRICS = ("cosine", "euclidean")
FN = {"cosine": "mi355rec_query_playlist_request_ext", "euclidean": "mi355rec_query_distance_request_ext"}
NODE_FN = {"cosine": "mi355rec_sharded_query_playlist_request_ext", "euclidean": "mi355rec_sharded_query_distance_request_ext"}
ONES = np.ones(12, np.float32)
check = distance_oracle.check   # equal ids, bit-equal scores or distances


def _call(eng, metric, rowset, mode, **kw):
    from spotify_recommender_amd import capi
    got = request_call(capi, getattr(eng._lib, FN[metric]), eng._h, metric, rowset._ptr() if rowset is not None else None, mode, **kw)
    assert got[0] == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return got[1], got[2]


def _engines(feats, always_without=False):
    """("replica off", engine) then ("replica on", engine), one alive at a time (tests/test_gpu_scaled.py); always_without: the first
    is created without a replica at every size (every row it admits takes the chains: rows_exact is then a function of the request)."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA if always_without or feats.shape[0] >= 65_536 else 0) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


def _values(metric, feats, members, a=ONES, weights=None):
    return distance_m(feats, members, a) if metric == "euclidean" else cosine_scores(feats, members, a, weights)


def _expected(metric, values, feats, gone, topn, where=None, labels=None, wanted=None):
    fn = distance_expected if metric == "euclidean" else cosine_expected
    return fn(values, feats, gone, topn, where, labels, wanted)


def _feats(n, seed=900):
    feats = oracle.mt19937_uniform(seed + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    return feats


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    feats = _feats(n)
    rng = np.random.default_rng(n)
    fixed = shapes(n)
    if n >= 4097:
        fixed["random5000"] = rng.integers(0, n, size=5000).astype(np.int64)     # (refused as an exclusion list: n_exclude > 1024)
    members = []
    for k in sorted({min(k, n) for k in (1, 3)}):
        rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = feats[int(rng.integers(0, n))]
        for metric in METRICS:
            for by, kw, mem, own in (("by row", dict(rows=rows), feats[rows], rows), ("by value", dict(members=vecs), vecs, [])):
                values = _values(metric, feats, mem)
                # the set-less request's own top-(1024 + 300): the best anchor rows and every row a threshold would have come from
                own_top = _expected(metric, values, feats, own, min(n, 1324))[0]
                members.append((k, metric, by, kw, own, values, own_top))
    wants = {}

    def want(i, sname, ids, mode):
        key = (i, sname, mode)
        if key not in wants:
            _, metric, _, _, own, values, _ = members[i]
            wants[key] = _expected(metric, values, feats, np.concatenate([np.asarray(own, np.int64), excluded(n, ids, mode)]), 1024)
        return wants[key]

    results = {}
    for replica, eng in _engines(feats):
        sets = {sname: eng.row_set(np.concatenate([ids, ids[:2]])) for sname, ids in fixed.items()}
        for sname, ids in fixed.items():
            assert sets[sname].count == np.unique(ids).size
        for i, (k, metric, by, kw, own, values, own_top) in enumerate(members):
            with eng.row_set(own_top) as top_set:
                for sname, ids, s in [(sname, fixed[sname], sets[sname]) for sname in fixed] + [("own_top", own_top, top_set)]:
                    for mname, mode in MODES:
                        w = want(i, sname, ids, mode)
                        for topn in TOPNS:
                            got = _call(eng, metric, s, mode, topn=topn, **kw)
                            check(got, prefix(w, topn), f"n={n} [{replica}] K={k} {metric} {by} {sname} {mname} top-{topn}")
                            results.setdefault((i, sname, mode, topn), []).append(got)
        for s in sets.values():
            s.close()
    for key, (off, on) in results.items():                        # replica on and off: identical results
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", COMPOSED)
def test_composition(engine_lib, n):
    """set + exclude + where + labels + signed weights; set + prior; set + diverse and set + capped (the MMR and caps oracles get
    the admissible pool); set + scales, cosine and euclidean."""
    from spotify_recommender_amd import capi
    feats = _feats(n, 300)
    rng = np.random.default_rng([2, n])
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    groups = rng.integers(-1, 40, size=n).astype(np.int32)
    priors = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    k = 3
    vecs = rng.random((k, 12), dtype=np.float32)
    rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
    signed = (rng.random(k, dtype=np.float32) + np.float32(0.1)) * np.asarray([1, -1, 1], np.float32)
    ex = [n - 1, 0, 0, 7]
    sc, sc_w, sc_r = cosine_scores(feats, vecs, ONES), cosine_scores(feats, vecs, ONES, signed), cosine_scores(feats, feats[rows], ONES)
    m_v = distance_m(feats, vecs, ONES)
    sc_s, m_s = cosine_scores(feats, vecs, GENERAL), distance_m(feats, vecs, GENERAL)
    fixed = {name: ids for name, ids in shapes(n).items() if name in ("even", "low_nibble", "mod4_is_1", "random30", "all_but_last")}
    fixed["own_top"] = cosine_expected(sc, feats, [], min(n, 400))[0]
    results = {}
    for replica, eng in _engines(feats):
        eng.set_labels(lab)
        eng.set_groups(groups)
        eng.set_priors(priors)
        fn = getattr(eng._lib, FN["cosine"])
        for sname, ids in fixed.items():
            with eng.row_set(ids) as s:
                for mname, mode in MODES:
                    what = f"n={n} [{replica}] {sname} {mname}"
                    gone = excluded(n, ids, mode, ex)
                    got = {}
                    got["all"] = _call(eng, "cosine", s, mode, members=vecs, weights=signed, exclude=ex, where=WHERE, labels=WANTED, topn=100)
                    check(got["all"], cosine_expected(sc_w, feats, gone, 100, WHERE, lab, WANTED), what + " exclude + where + labels + weights")
                    got["dist"] = _call(eng, "euclidean", s, mode, members=vecs, exclude=ex, where=WHERE, labels=WANTED, topn=100)
                    check(got["dist"], distance_expected(m_v, feats, gone, 100, WHERE, lab, WANTED), what + " distance, composed")
                    rc, gi, gs, _, _ = request_call(capi, fn, eng._h, "cosine", s._ptr(), mode, rows=rows, exclude=ex, topn=100, prior_weight=-0.5)
                    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                    got["prior"] = (gi, gs)
                    check(got["prior"], prior_oracle.expected_prior(sc_r, priors, -0.5, feats, None, None, np.concatenate([rows, gone]), 100),
                          what + " prior")
                    for topn, pool in ((10, 40), (100, 1024)):
                        pool_rows = playlist_labels_oracle.expected_scored(sc, feats, None, None, gone, pool)
                        rc, gi, gs, gm, _ = request_call(capi, fn, eng._h, "cosine", s._ptr(), mode, members=vecs, exclude=ex, topn=topn, lam=0.6, pool=pool)
                        assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                        wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, topn)
                        check((gi, gs), (wi, ws), what + f" diverse top-{topn} of {pool}")
                        assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), what + " mmr"
                        rc, gi, gs, gm, p_rows = request_call(capi, fn, eng._h, "cosine", s._ptr(), mode, members=vecs, exclude=ex, topn=topn,
                                                              lam=0.6, pool=pool, max_per_group=2)
                        assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                        wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, topn, groups, 2)
                        check((gi, gs), (wi, ws), what + f" capped top-{topn} of {pool}")
                        assert p_rows == pool_rows[0].size
                        got[f"capped{topn}"] = (gi, gs)
                    got["scaled"] = _call(eng, "cosine", s, mode, members=vecs, exclude=ex, scales=GENERAL, topn=100)
                    check(got["scaled"], cosine_expected(sc_s, feats, gone, 100), what + " scales, cosine")
                    got["scaled_dist"] = _call(eng, "euclidean", s, mode, members=vecs, exclude=ex, scales=GENERAL, topn=100)
                    check(got["scaled_dist"], distance_expected(m_s, feats, gone, 100), what + " scales, euclidean")
                    for key, v in got.items():
                        results.setdefault((sname, mode, key), []).append(v)
    for key, (off, on) in results.items():
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [257, 4097])
def test_identities(engine_lib, n):
    """ext == NULL and an ext of two NULL pointers are the plain request (same launch: the same rows_exact), scales only is the
    _scaled call, EXCLUDE with |S| <= 1024 is S appended to exclude_global, EXCLUDE with an empty set is the plain request, ONLY with an
    empty set and EXCLUDE with every row answer count 0 without a launch."""
    from spotify_recommender_amd import capi
    feats = _feats(n, 500)
    rng = np.random.default_rng([8, n])
    vecs = rng.random((3, 12), dtype=np.float32)
    small = rng.choice(n, size=min(n - 20, 700), replace=False).astype(np.int64)
    plain = {"cosine": ("mi355rec_query_playlist_request", playlist_labels_oracle.request_call),
             "euclidean": ("mi355rec_query_distance_request", distance_oracle.request_call)}
    scaled = {"cosine": "mi355rec_query_playlist_request_scaled", "euclidean": "mi355rec_query_distance_request_scaled"}
    for replica, eng in _engines(feats, always_without=True):
        with eng.row_set(small) as s, eng.row_set([]) as empty, eng.row_set(np.arange(n)) as full:
            assert (s.count, empty.count, full.count) == (small.size, 0, n)
            for metric in METRICS:
                name, req = plain[metric]
                fn = getattr(eng._lib, FN[metric])
                for kw in (dict(rows=[5, 9]), dict(members=vecs, exclude=[1, 2], where=WHERE)):
                    c0 = eng.playlist_counters()
                    want = req(capi, getattr(eng._lib, name), eng._h, topn=100, **kw)[1:3]
                    c1 = eng.playlist_counters()
                    for what, rowset, mode, more in (("NULL ext", None, 0, dict(ext_null=True)), ("two NULL pointers", None, 7, {}),
                                                     ("EXCLUDE, empty set", empty, EXCLUDE, {}), ("ONLY, every row", full, ONLY, {})):
                        before = eng.playlist_counters()
                        got = request_call(capi, fn, eng._h, metric, rowset._ptr() if rowset else None, mode, topn=100, **more, **kw)
                        after = eng.playlist_counters()
                        assert got[0] == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                        check(got[1:3], want, f"[{replica}] {metric} {what}")
                        if replica == "replica off":              # the same launch: the same rows take the chains
                            assert after["rows_exact"] - before["rows_exact"] == c1["rows_exact"] - c0["rows_exact"], what
                    for what, rowset, mode in (("ONLY, empty set", empty, ONLY), ("EXCLUDE, every row", full, EXCLUDE)):
                        before = eng.playlist_counters()
                        got = request_call(capi, fn, eng._h, metric, rowset._ptr(), mode, topn=100, **kw)
                        after = eng.playlist_counters()
                        assert got[0] == capi.OK and got[1].size == 0, what
                        assert after["rows_exact"] == before["rows_exact"] and after["queries"] == before["queries"] + 1, what   # no launch

                    def with_scales(handle, query, result, metric=metric):
                        return getattr(eng._lib, scaled[metric])(handle, query, GENERAL.ctypes.data_as(ctypes.c_void_p), result)
                    got = request_call(capi, fn, eng._h, metric, None, 0, scales=GENERAL, topn=100, **kw)
                    assert got[0] == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                    check(got[1:3], req(capi, with_scales, eng._h, topn=100, **kw)[1:3], f"[{replica}] {metric} scales only")
                    kw_x = dict(kw, exclude=list(kw.get("exclude", [])) + small.tolist())
                    got = request_call(capi, fn, eng._h, metric, s._ptr(), EXCLUDE, topn=100, **kw)
                    assert got[0] == capi.OK, eng._lib.mi355rec_last_error(eng._h)
                    check(got[1:3], req(capi, getattr(eng._lib, name), eng._h, topn=100, **kw_x)[1:3], f"[{replica}] {metric} S appended to exclude_global")


def test_the_5000_id_history_is_refused_as_an_exclusion_list(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    n = 4097
    feats = _feats(n)
    ids = np.random.default_rng(1).integers(0, n, size=5000)
    with CosineEngine(feats) as eng:
        with pytest.raises(capi.Mi355Error, match="n_exclude 5000"):
            eng.query_mean_topn(feats[:1], 10, exclude=ids.tolist())
        got = eng.query_mean_topn(feats[:1], 10, seen=ids)
        check(got, cosine_expected(cosine_scores(feats, feats[:1], ONES), feats, ids, 10), "5000 ids as seen=")


@pytest.mark.parametrize("n", [2049, 65_537])
def test_add_and_lanes(engine_lib, n):
    """Creating from half the ids and adding the rest (with duplicates) equals creating from all; a set made on the parent answers
    the same on a lane; the Python forms."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = _feats(n, 40)
    rng = np.random.default_rng([12, n])
    ids = rng.choice(n, size=n // 3, replace=False).astype(np.int64)
    half = ids.size // 2
    vecs = rng.random((2, 12), dtype=np.float32)
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        lane = eng.lane()
        try:
            with eng.row_set(ids) as whole, eng.row_set(ids[:half]) as grown:
                assert grown.count == half
                first = {(metric, mode): _call(eng, metric, grown, mode, members=vecs, topn=100) for metric in METRICS for _, mode in MODES}
                grown.add(np.concatenate([ids[half - 7:], ids[:10], ids[-5:]]))      # the rest, with duplicates
                assert grown.count == whole.count == ids.size
                with pytest.raises(capi.Mi355Error, match="id -3"):
                    grown.add([1, -3])
                assert grown.count == ids.size
                for metric in METRICS:
                    values = _values(metric, feats, vecs)
                    for mname, mode in MODES:
                        want = _expected(metric, values, feats, excluded(n, ids, mode), 100)
                        check(_call(eng, metric, grown, mode, members=vecs, topn=100), want, f"n={n} {metric} {mname}: grown")
                        check(_call(eng, metric, whole, mode, members=vecs, topn=100), want, f"n={n} {metric} {mname}: whole")
                        check(_call(lane, metric, whole, mode, members=vecs, topn=100), want, f"n={n} {metric} {mname}: on a lane")
                        check(first[(metric, mode)], _expected(metric, values, feats, excluded(n, ids[:half], mode), 100), "before the add")
                comp = np.setdiff1d(np.arange(n), ids)
                a = eng.query_mean_topn(vecs, 20, seen=whole)
                check(eng.query_mean_topn(vecs, 20, only=comp), a, "only= the complement, a plain sequence")
                check(lane.query_mean_topn(vecs, 20, seen=whole), a, "the Python method on a lane")
                check(eng.query_nearest_rows_scaled([3, 4], 20, None, seen=ids), eng.query_nearest_rows_scaled([3, 4], 20, None, only=comp), "nearest")
                with pytest.raises(ValueError, match="mutually exclusive"):
                    eng.query_playlist_topn([1], 5, seen=whole, only=whole)
        finally:
            lane.close()


@pytest.mark.parametrize("n", [2049, 65_537])
def test_rows_exact_says_the_test_precedes_the_chains(engine_lib, n):
    """Replica off, no filter, no exclusion list, members by value: one request computes the chains of exactly the rows the set
    admits: n - count (EXCLUDE) or count (ONLY)."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = _feats(n, 60)
    vecs = np.random.default_rng(n).random((3, 12), dtype=np.float32)
    fixed = shapes(n)
    fixed["one_percent"] = np.random.default_rng(5).choice(n, size=max(n // 100, 1), replace=False)
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA) as eng:
        for sname, ids in fixed.items():
            with eng.row_set(ids) as s:
                for mname, mode in MODES:
                    for metric in METRICS:
                        before = eng.playlist_counters()["rows_exact"]
                        _call(eng, metric, s, mode, members=vecs, topn=10)
                        delta = eng.playlist_counters()["rows_exact"] - before
                        assert delta == (n - s.count if mode == EXCLUDE else s.count), (sname, mname, metric, delta, s.count)


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handle(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 10_007
    feats = _feats(n, 10)
    feats[n // 2 - 2:n // 2 + 2] = feats[17]                      # ties across the two shards
    rng = np.random.default_rng(10)
    vecs = rng.random((3, 12), dtype=np.float32)
    rows = [17, 5003, 5004]
    place = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    fixed = {name: ids for name, ids in shapes(n).items() if name in ("even", "low_nibble", "random30", "last_only")}
    fixed["second_shard"] = np.arange(5004, n, dtype=np.int64)
    fixed["random5000"] = rng.integers(0, n, size=5000).astype(np.int64)
    with NodeEngine(feats, devices=[0, 0], placement=place) as node, CosineEngine(feats) as eng:
        info = node.info()
        if placement == "sharded":
            assert info["shard_rows"] == [5004, 5003] and info["shard_rows"][0] % 8 != 0   # the second shard's slice starts inside a byte
        for sname, ids in fixed.items():
            with node.row_set(ids) as ns, eng.row_set(ids) as es:
                assert ns.count == es.count == np.unique(ids).size
                for mname, mode in MODES:
                    what = f"{placement} {sname} {mname}"
                    for metric in METRICS:
                        for kw, own in ((dict(rows=rows, exclude=[1, 9000]), rows), (dict(members=vecs), [])):
                            got = request_call(capi, getattr(node._lib, NODE_FN[metric]), node._h, metric, ns._ptr(), mode, topn=100, **kw)
                            assert got[0] == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                            check(got[1:3], _call(eng, metric, es, mode, topn=100, **kw), what + f" {metric}: against the single handle")
                            mem = feats[rows] if "rows" in kw else vecs
                            gone = excluded(n, ids, mode, list(kw.get("exclude", [])) + own)
                            check(got[1:3], _expected(metric, _values(metric, feats, mem), feats, gone, 100), what + f" {metric}")
                    got = request_call(capi, getattr(node._lib, NODE_FN["cosine"]), node._h, "cosine", ns._ptr(), mode, members=vecs, topn=10,
                                       lam=0.6, pool=40)
                    assert got[0] == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                    want = request_call(capi, getattr(eng._lib, FN["cosine"]), eng._h, "cosine", es._ptr(), mode, members=vecs, topn=10, lam=0.6, pool=40)
                    check(got[1:3], want[1:3], what + " diverse")
                    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
                    pool_rows = playlist_labels_oracle.expected_scored(cosine_scores(feats, vecs, ONES), feats, None, None, excluded(n, ids, mode), 40)
                    check(got[1:3], playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, 10)[:2], what + " diverse against the oracle")
                if sname == "even":
                    half = ids[: ids.size // 2]
                    with node.row_set(half) as grown:
                        grown.add(ids[ids.size // 2 - 3:])
                        assert grown.count == ns.count
                        check(node.query_mean_topn(vecs, 50, only=grown), node.query_mean_topn(vecs, 50, only=ns), placement + " add")
                    # a single-handle set on a node handle, and the reverse
                    rc = request_call(capi, getattr(node._lib, NODE_FN["cosine"]), node._h, "cosine", es._ptr(), 0, members=vecs, topn=5)[0]
                    assert rc == capi.ERR_INVALID_ARG and "row set of another handle" in node._lib.mi355rec_sharded_last_error(node._h).decode()
                    rc = request_call(capi, getattr(eng._lib, FN["euclidean"]), eng._h, "euclidean", ns._ptr(), 1, members=vecs, topn=5)[0]
                    assert rc == capi.ERR_INVALID_ARG and "row set of another handle" in eng._lib.mi355rec_last_error(eng._h).decode()
        check(node.query_playlist_topn([3, 4], 20, seen=fixed["even"]), eng.query_playlist_topn([3, 4], 20, seen=fixed["even"]), "the Python methods")


def test_a_set_of_another_single_handle_is_refused(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = _feats(257)
    with CosineEngine(feats) as a, CosineEngine(feats) as b, a.row_set([1, 2]) as s:
        with pytest.raises(capi.Mi355Error, match="row set of another handle"):
            b.query_mean_topn(feats[:1], 5, seen=s)
        out = ctypes.c_void_p()
        bad = np.asarray([2 ** 32], np.int64)
        assert a._lib.mi355rec_rowset_create(a._h, bad.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(out)) == capi.ERR_INVALID_ARG
        assert "id 4294967296" in a._lib.mi355rec_last_error(a._h).decode()
        with a.row_set([2 ** 32 - 1, 300, 5]) as wide:           # ids outside [row_base, row_base + n) match nothing
            assert wide.count == 1
