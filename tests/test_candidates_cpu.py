"""CANDIDATE LISTS on a host without a GPU (include/mi355rec_diag.h): the node-handle _candidates entry points served by the
product's CPU backend against tests/candidates_oracle.py (the existing oracles with exclude + the complement of the list) — equal
ids, bit-equal scores and distances, counts and padding — the identities of the header, every argument error with its message, the
Python form on both engines, and csrc/candidates.h itself in a stand-alone program (tests/candidates_check.cpp) under
AddressSanitizer and UBSan, run as its own process."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import distance_oracle, playlist_labels_oracle, prior_oracle, rowset_oracle
from tests.candidates_oracle import gone, request_call
from tests.playlist_labels_oracle import uniform_labels
from tests.rowset_oracle import EXCLUDE, ONLY, prefix
from tests.scaled_oracle import GENERAL, cosine_expected, cosine_scores, distance_expected, distance_m

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
METRICS = ("cosine", "euclidean")
FN = {"cosine": "mi355rec_sharded_query_playlist_request_candidates", "euclidean": "mi355rec_sharded_query_distance_request_candidates"}
EXT_FN = {"cosine": "mi355rec_sharded_query_playlist_request_ext", "euclidean": "mi355rec_sharded_query_distance_request_ext"}
PLAIN = {"cosine": ("mi355rec_sharded_query_playlist_request", playlist_labels_oracle.request_call),
         "euclidean": ("mi355rec_sharded_query_distance_request", distance_oracle.request_call)}
ONES = np.ones(12, np.float32)
check = distance_oracle.check


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


def _err(nd):
    return nd._lib.mi355rec_sharded_last_error(nd._h).decode()


def _call(nd, metric, cand, rowset=None, mode=0, **kw):
    from spotify_recommender_amd import capi
    got = request_call(capi, getattr(nd._lib, FN[metric]), nd._h, metric, cand, rowset._ptr() if rowset is not None else None, mode, **kw)
    assert got[0] == capi.OK, _err(nd)
    return got[1], got[2]


def _values(metric, feats, members, a=ONES, weights=None):
    return distance_m(feats, members, a) if metric == "euclidean" else cosine_scores(feats, members, a, weights)


def _expected(metric, values, feats, out, topn, where=None, labels=None, wanted=None):
    fn = distance_expected if metric == "euclidean" else cosine_expected
    return fn(values, feats, out, topn, where, labels, wanted)


def _feats(n):
    from oracle import oracle
    feats = oracle.mt19937_uniform(800 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]
        feats[n // 2] = feats[3]
    return feats


def _lists(n, rng):
    """name -> ids: in any order, with duplicates, the ends of the catalogue."""
    r = np.arange(n, dtype=np.int64)
    some = rng.permutation(r[rng.random(n) < 0.3])
    return {"empty": r[:0], "one": r[-1:], "ends": np.asarray([n - 1, 0, n - 1], np.int64), "every row": r, "descending": r[::-1][: max(n // 2, 1)],
            "shuffled 30 % with duplicates": np.concatenate([some, some[:5]])}


@cpu_only
@pytest.mark.parametrize("n", [1, 5, 257, 2049])
def test_parity(engine_lib, n):
    feats = _feats(n)
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    with _node(feats) as nd:
        nd.set_labels(lab)
        for k in sorted({min(k, n) for k in (1, 3)}):
            rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
            vecs = rng.random((k, 12), dtype=np.float32)
            signed = (rng.random(k, dtype=np.float32) + np.float32(0.1)) * np.where(np.arange(k) % 3 == 1, -1, 1).astype(np.float32)
            for metric in METRICS:
                v_r, v_v = _values(metric, feats, feats[rows]), _values(metric, feats, vecs)
                for lname, ids in _lists(n, rng).items():
                    what = f"n={n} K={k} {metric} {lname}"
                    out = gone(n, ids)
                    want_r = _expected(metric, v_r, feats, np.concatenate([rows, out]), 1024)
                    want_v = _expected(metric, v_v, feats, out, 1024)
                    for topn in (1, 10, 1024):
                        check(_call(nd, metric, ids, rows=rows, topn=topn), prefix(want_r, topn), what + " by row")
                        check(_call(nd, metric, ids, members=vecs, topn=topn), prefix(want_v, topn), what + " by value")
                    ex = [n - 1, 0, 0]
                    check(_call(nd, metric, ids, members=vecs, exclude=ex, where=WHERE, labels=WANTED, topn=10),
                          _expected(metric, v_v, feats, gone(n, ids, ex), 10, WHERE, lab, WANTED), what + " exclude + where + labels")
                    if metric == "cosine":
                        v_w = _values(metric, feats, vecs, weights=signed)
                        check(_call(nd, metric, ids, members=vecs, weights=signed, exclude=[0], topn=10),
                              _expected(metric, v_w, feats, gone(n, ids, [0]), 10), what + " signed weights")
                    check(_call(nd, metric, ids, members=vecs, scales=GENERAL, topn=10),
                          _expected(metric, _values(metric, feats, vecs, GENERAL), feats, out, 10), what + " scaled")


@cpu_only
def test_prior_diverse_and_capped_get_the_listed_pool(engine_lib):
    from spotify_recommender_amd import capi
    n = 2049
    feats = _feats(n)
    rng = np.random.default_rng([4, n])
    groups = rng.integers(-1, 12, size=n).astype(np.int32)
    priors = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    vecs = rng.random((3, 12), dtype=np.float32)
    sc = playlist_labels_oracle.scores_of(feats, vecs)
    fn = getattr(capi.lib(), FN["cosine"])
    ids = rng.permutation(n)[:600].astype(np.int64)
    with _node(feats) as nd:
        nd.set_groups(groups)
        nd.set_priors(priors)
        out = gone(n, ids, [1])
        rc, gi, gs, _, _ = request_call(capi, fn, nd._h, "cosine", ids, members=vecs, exclude=[1], topn=10, prior_weight=0.75)
        assert rc == capi.OK, _err(nd)
        check((gi, gs), prior_oracle.expected_prior(sc, priors, 0.75, feats, None, None, out, 10), "prior")
        for topn, pool in ((5, 5), (10, 40)):
            pool_rows = playlist_labels_oracle.expected_scored(sc, feats, None, None, out, pool)
            rc, gi, gs, gm, _ = request_call(capi, fn, nd._h, "cosine", ids, members=vecs, exclude=[1], topn=topn, lam=0.6, pool=pool)
            assert rc == capi.OK, _err(nd)
            wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, topn)
            check((gi, gs), (wi, ws), f"diverse top-{topn} of {pool}")
            assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32))
            rc, gi, gs, gm, p_rows = request_call(capi, fn, nd._h, "cosine", ids, members=vecs, exclude=[1], topn=topn, lam=0.6, pool=pool,
                                                  max_per_group=2)
            assert rc == capi.OK, _err(nd)
            wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, topn, groups, 2)
            check((gi, gs), (wi, ws), f"capped top-{topn} of {pool}")
            assert p_rows == pool_rows[0].size


@cpu_only
def test_identities(engine_lib):
    """list == ONLY row set of the same ids; list + EXCLUDE set == ONLY set of C minus S; list + ONLY set == ONLY set of C and S; the
    full list == the plain request; members may be listed and are never returned; an empty list answers count 0."""
    from spotify_recommender_amd import capi
    n = 2049
    feats = _feats(n)
    rng = np.random.default_rng(8)
    vecs = rng.random((3, 12), dtype=np.float32)
    C = rng.permutation(n)[:700].astype(np.int64)
    S = rng.permutation(n)[:900].astype(np.int64)
    with _node(feats) as nd, nd.row_set(C) as only_c, nd.row_set(S) as s, nd.row_set(np.setdiff1d(C, S)) as c_minus_s, \
            nd.row_set(np.intersect1d(C, S)) as c_and_s:
        for metric in METRICS:
            ext = getattr(nd._lib, EXT_FN[metric])
            name, req = PLAIN[metric]
            for kw in (dict(rows=[int(C[0]), int(C[1])]), dict(members=vecs, exclude=[1, 2], where=WHERE)):
                def with_set(rowset, kw=kw, ext=ext, metric=metric):
                    got = rowset_oracle.request_call(capi, ext, nd._h, metric, rowset._ptr(), ONLY, topn=100, **kw)
                    assert got[0] == capi.OK, _err(nd)
                    return got[1:3]
                check(_call(nd, metric, C, topn=100, **kw), with_set(only_c), f"{metric}: list against the ONLY set")
                check(_call(nd, metric, C, s, EXCLUDE, topn=100, **kw), with_set(c_minus_s), f"{metric}: list + EXCLUDE set")
                check(_call(nd, metric, C, s, ONLY, topn=100, **kw), with_set(c_and_s), f"{metric}: list + ONLY set")
                want = req(capi, getattr(nd._lib, name), nd._h, topn=100, **kw)[1:3]
                check(_call(nd, metric, np.arange(n), topn=100, **kw), want, f"{metric}: the full list against the plain request")
                check(_call(nd, metric, np.arange(n), ext_null=True, topn=100, **kw), want, f"{metric}: ... with a NULL ext")
                got = _call(nd, metric, [], topn=100, **kw)
                assert got[0].size == 0
            got = _call(nd, metric, C[:2], rows=[int(C[0]), int(C[1])], topn=5)      # every candidate is a member
            assert got[0].size == 0
            got = _call(nd, metric, C[:3], members=vecs, exclude=C[:3].tolist(), topn=5)   # ... or excluded
            assert got[0].size == 0


@cpu_only
def test_padding_and_count(engine_lib):
    from spotify_recommender_amd import capi
    n = 257
    feats = _feats(n)
    L = capi.lib()
    vecs = feats[:2].copy()
    with _node(feats) as nd:
        for metric in METRICS:
            q = (capi.DistanceQuery if metric == "euclidean" else capi.PlaylistQuery)()
            q.size = ctypes.sizeof(q)
            q.members, q.k, q.topn = vecs.ctypes.data_as(ctypes.c_void_p), 2, 10
            idx, score, count = np.full(10, 99, np.int64), np.full(10, 9.0, np.float32), ctypes.c_int(77)
            if metric == "euclidean":
                res = capi.DistanceResult(idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p), ctypes.pointer(count))
            else:
                res = capi.PlaylistResult(idx.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p), None, ctypes.pointer(count), None)
            cand = np.asarray([200, 7, 7, 100], np.int64)
            assert getattr(L, FN[metric])(nd._h, ctypes.byref(q), None, cand.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(res)) == capi.OK
            assert count.value == 3 and sorted(idx[:3].tolist()) == [7, 100, 200]
            assert idx[3:].tolist() == [-1] * 7 and score[3:].tolist() == [0.0] * 7
            assert getattr(L, FN[metric])(nd._h, ctypes.byref(q), None, None, 0, ctypes.byref(res)) == capi.OK       # an empty list
            assert count.value == 0 and idx.tolist() == [-1] * 10 and score.tolist() == [0.0] * 10


@cpu_only
def test_refusals(engine_lib):
    from spotify_recommender_amd import capi
    n = 257
    feats = _feats(n)
    vecs = feats[:2]
    L = capi.lib()
    with _node(feats) as nd, _node(feats[:100]) as other, other.row_set([1]) as foreign:
        for metric in METRICS:
            fn = getattr(L, FN[metric])
            for cand, more, msg in (([3, -1], {}, "candidate list: id -1 out of [0, 257)"),
                                    ([257], {}, "candidate list: id 257 out of [0, 257)"),
                                    ([1], dict(n_candidates=-1), "candidate list: n_candidates must not be negative, got -1"),
                                    ([1, 2], dict(null_list=True), "candidate list: null list with n_candidates 2"),
                                    ([1], dict(n_candidates=capi.MAX_CANDIDATES + 1),
                                     "candidate list: n_candidates 1048577 above MI355REC_MAX_CANDIDATES (1048576)")):
                rc = request_call(capi, fn, nd._h, metric, cand, members=vecs, topn=5, **more)[0]
                assert rc == capi.ERR_INVALID_ARG and _err(nd) == msg, (metric, msg, _err(nd))
            # every check of the _ext call comes first, with its message
            for more, msg in ((dict(ext_size=32), "request ext of size 32"), (dict(ext_size=0), "request ext of size 0"),
                              (dict(scales=np.full(12, np.nan, np.float32)), "feature scale 0 is nan")):
                rc = request_call(capi, fn, nd._h, metric, [3, -1], members=vecs, topn=5, **more)[0]
                assert rc == capi.ERR_INVALID_ARG and msg in _err(nd), (metric, msg, _err(nd))
            rc = request_call(capi, fn, nd._h, metric, [3], foreign._ptr(), 0, members=vecs, topn=5)[0]
            assert rc == capi.ERR_INVALID_ARG and "row set of another handle" in _err(nd)
            rc = request_call(capi, fn, nd._h, metric, [3], members=vecs, topn=0)[0]
            assert rc == capi.ERR_INVALID_ARG and "topn" in _err(nd)
        assert getattr(L, FN["cosine"])(None, None, None, None, 0, None) == capi.ERR_INVALID_ARG
        full = np.zeros(capi.MAX_CANDIDATES, np.int64)                            # exactly the maximum is served
        got = _call(nd, "cosine", full, members=vecs, topn=5)
        assert got[0].tolist() == [0]


@cpu_only
def test_python_form(engine_lib):
    from spotify_recommender_amd.engine import with_candidates
    n = 2049
    feats = _feats(n)
    rng = np.random.default_rng(12)
    ids = rng.permutation(n)[:900].astype(np.int64)
    hist = rng.permutation(n)[:500].astype(np.int64)
    vecs = rng.random((2, 12), dtype=np.float32)
    with _node(feats) as nd:
        nd.set_groups(np.arange(n, dtype=np.int32) % 7)
        view = with_candidates(nd, ids.tolist())                                 # a plain sequence; an int64 array below
        check(view.query_mean_topn(vecs, 20), nd.query_mean_topn(vecs, 20, only=ids), "query_mean_topn")
        check(with_candidates(nd, ids).query_playlist_topn([3, 4], 20), nd.query_playlist_topn([3, 4], 20, only=ids), "query_playlist_topn")
        check(view.query_mean_topn(vecs, 20, seen=hist), nd.query_mean_topn(vecs, 20, only=np.setdiff1d(ids, hist)), "with seen=")
        check(view.query_mean_topn(vecs, 20, only=hist), nd.query_mean_topn(vecs, 20, only=np.intersect1d(ids, hist)), "with only=")
        check(view.query_nearest(vecs, 20), nd.query_nearest_scaled(vecs, 20, None, only=ids), "query_nearest")
        check(view.query_nearest_rows([3, 4], 20), nd.query_nearest_rows_scaled([3, 4], 20, None, only=ids), "query_nearest_rows")
        check(view.query_nearest_scaled(vecs, 20, GENERAL, seen=hist),
              nd.query_nearest_scaled(vecs, 20, GENERAL, only=np.setdiff1d(ids, hist)), "query_nearest_scaled")
        check(view.query_mean_topn(vecs, 20, scales=GENERAL, where=WHERE), nd.query_mean_topn(vecs, 20, scales=GENERAL, where=WHERE, only=ids), "scaled")
        d = view.query_mean_topn_diverse(vecs, 10, 0.5, return_mmr=True)
        e = nd.query_mean_topn_diverse(vecs, 10, 0.5, only=ids, return_mmr=True)
        assert all(np.array_equal(x, y) for x, y in zip(d, e))
        d = view.query_playlist_topn_capped([3, 4], 10, 1, return_pool_rows=True)
        e = nd.query_playlist_topn_capped([3, 4], 10, 1, only=ids, return_pool_rows=True)
        assert all(np.array_equal(x, y) for x, y in zip(d, e))
        assert with_candidates(nd, []).query_mean_topn(vecs, 20)[0].size == 0
        check(nd.query_mean_topn(vecs, 20), with_candidates(nd, np.arange(n)).query_mean_topn(vecs, 20), "the engine itself is left as it was")
        with pytest.raises(AttributeError, match="candidate list"):
            view.query_row_topn(3, 5)


def test_constants_and_bindings(engine_lib):
    from spotify_recommender_amd import capi
    header = (ROOT / "include" / "mi355rec_diag.h").read_text()
    assert f"#define MI355REC_MAX_CANDIDATES {capi.MAX_CANDIDATES}\n" in header and capi.MAX_CANDIDATES == 1_048_576
    assert ctypes.sizeof(capi.RequestExt) == 24
    for name in list(FN.values()) + [v.replace("sharded_", "") for v in FN.values()] + ["mi355rec_candidates_counters"]:
        assert name in capi.SIGNATURES and hasattr(engine_lib, name) and name + "(" in header, name


@pytest.fixture(scope="module")
def candidates_check(tmp_path_factory):
    """tests/candidates_check.cpp built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("candidates") / "candidates_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           str(ROOT / "tests" / "candidates_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_candidates_h_under_sanitizers(candidates_check):
    p = subprocess.run([str(candidates_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "candidates.h: ok" in p.stdout, p.stdout + p.stderr
