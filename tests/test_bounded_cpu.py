"""BOUNDED REQUESTS on a host without a GPU (include/mi355rec_diag.h): mi355rec_sharded_query_bounded_request served by the product's
CPU backend (csrc/cpu_backend.cpp) against tests/bounded_oracle.py — equal ids, bit-equal values, equal totals, the padding — plus
every refusal of the new struct with its code and whole text, the short structs and the bindings."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import bounded_oracle as bo
from tests.distance_oracle import hostile_catalogue
from tests.playlist_labels_oracle import uniform_labels


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

SIZES = (1, 3, 4, 5, 2047, 2048, 2049, 4097)
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [1, 4, 4, 9]


def _call(nd, **kw):
    from spotify_recommender_amd import capi
    rc, ids, sc, total = bo.request_call(capi, nd._lib.mi355rec_sharded_query_bounded_request, nd._h, **kw)
    assert rc == capi.OK, nd._lib.mi355rec_sharded_last_error(nd._h)
    return ids, sc, total


def _refused(nd, text, **kw):
    from spotify_recommender_amd import capi
    rc = bo.request_call(capi, nd._lib.mi355rec_sharded_query_bounded_request, nd._h, **kw)[0]
    assert rc == capi.ERR_INVALID_ARG, (rc, kw)
    assert nd._lib.mi355rec_sharded_last_error(nd._h).decode() == text


@pytest.mark.parametrize("n", SIZES)
def test_parity(engine_lib, n):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(n)
    lab = uniform_labels(n, 12, 3, unlabelled=0.05)
    rng = np.random.default_rng([7, n])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(lab)
        for k in (1, 2, 32):
            rows = [int(r) for r in rng.choice(n, size=min(k, n), replace=False)]
            if 0 not in rows:
                rows[0] = 0                                          # row 0 has duplicates: distance 0, ties by row
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            excl = [0, 0, n // 2, n - 1]
            for metric in (bo.COSINE, bo.EUCLIDEAN):
                for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []), ("by row", dict(rows=rows), feats[rows], rows)):
                    v = bo.values(feats, members, metric)
                    ok = bo.admissible(feats, v, excluded)
                    ok_all = bo.admissible(feats, v, excluded + excl, WHERE, lab, WANTED)
                    for bound in bo.bounds_for(v, ok, metric):
                        total = bo.expected_from_values(v, ok, metric, bound, 0)[2]
                        for topn in bo.topns_for(total):
                            tag = f"n={n} k={k} metric={metric} {what} bound={bound!r} top-{topn}"
                            bo.check(_call(nd, metric=metric, bound=bound, topn=topn, **kw), bo.expected_from_values(v, ok, metric, bound, topn), tag)
                        bo.check(_call(nd, metric=metric, bound=bound, topn=10, exclude=excl, where=WHERE, labels=WANTED, **kw),
                                 bo.expected_from_values(v, ok_all, metric, bound, 10), tag + " all together")


def test_zero_floor_of_either_sign_on_a_catalogue_with_zero_rows(engine_lib):
    """A zero row scores +0.0 against any member (den <= 1e-8): it matches a floor of +0.0 and of -0.0 alike."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 300
    feats = (np.random.default_rng(3).random((n, 12), dtype=np.float32) - np.float32(0.5))
    feats[[5, 77, 299]] = 0.0
    v = bo.values(feats, feats[[1, 2]], bo.COSINE)
    ok = bo.admissible(feats, v, [1, 2])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        plus = _call(nd, rows=[1, 2], bound=0.0, topn=1024)
        minus = _call(nd, rows=[1, 2], bound=-0.0, topn=1024)
        bo.check(plus, bo.expected_from_values(v, ok, bo.COSINE, 0.0, 1024), "+0.0")
        bo.check(minus, plus, "-0.0 against +0.0")
        assert {5, 77, 299} <= set(plus[0].tolist())


def test_radius_zero_counts_the_duplicates(engine_lib):
    from spotify_recommender_amd import capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(257)
    dups = [i for i in range(257) if np.array_equal(feats[i], feats[0])]
    assert len(dups) >= 5
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        ids, dist, total = _call(nd, metric=bo.EUCLIDEAN, members=feats[:1], bound=0.0, topn=100)
        assert ids.tolist() == dups and total == len(dups) and not dist.view(np.uint32).any()
        ids, dist, total = _call(nd, metric=bo.EUCLIDEAN, rows=[0], bound=0.0, topn=100)      # the member row itself is never counted
        assert ids.tolist() == dups[1:] and total == len(dups) - 1
        got = engine.query_bounded(nd, 3, 0.0, metric="euclidean", rows=[0])
        assert got[0].tolist() == dups[1:4] and got[2] == len(dups) - 1
        assert engine.query_bounded(nd, 0, 0.0, metric="euclidean", members=feats[:1])[2] == len(dups)


def test_the_python_function_with_row_sets(engine_lib):
    from spotify_recommender_amd import capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 4097
    feats = np.random.default_rng(11).random((n, 12), dtype=np.float32)
    seen = sorted({int(r) for r in np.random.default_rng(12).choice(n, size=n // 3, replace=False)})
    v = bo.values(feats, feats[[3, 4]], bo.COSINE)
    bound = float(np.sort(v)[n // 2])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        for kw, rs in ((dict(seen=seen), False), (dict(only=seen), True)):
            ok = bo.admissible(feats, v, [3, 4, 9], rowset=seen, rowset_only=rs)
            bo.check(engine.query_bounded(nd, 50, bound, rows=[3, 4], exclude=[9], **kw), bo.expected_from_values(v, ok, bo.COSINE, bound, 50), str(kw))
        with pytest.raises(ValueError):
            engine.query_bounded(nd, 5, 0.5)
        with pytest.raises(ValueError):
            engine.query_bounded(nd, 5, 0.5, metric="manhattan", rows=[1])


def test_refusals_code_and_whole_text(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 64
    feats = np.random.default_rng(1).random((n, 12), dtype=np.float32)
    one = feats[:1]
    size = ctypes.sizeof(capi.BoundedQuery)
    assert size == 72 and capi.BoundedQuery.metric.offset == 64 and capi.BoundedQuery.bound.offset == 68
    scales = np.ones(12, np.float32)
    ext = capi.RequestExt(ctypes.sizeof(capi.RequestExt), 0, scales.ctypes.data_as(ctypes.c_void_p), None)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        for bad in (0, 3, 7, 70, 73, 80):
            _refused(nd, f"bounded query of size {bad}: not the end of a field of the 72 bytes this library reads", members=one, size=bad)
        _refused(nd, "flags 0x1 in a bounded query: must be 0 (weights, diversified and capped calls and priors are not served)", members=one, flags=1)
        _refused(nd, "members by value and by row in one bounded query", members=one, rows=[1])
        _refused(nd, "a bounded query needs members by value or by row")
        _refused(nd, "a bounded query needs members by value or by row", members=one, size=8)       # cut before the members
        _refused(nd, "metric 2 in a bounded query: MI355REC_BOUNDED_COSINE (0) or MI355REC_BOUNDED_EUCLIDEAN (1)", members=one, metric=2)
        _refused(nd, "metric -1 in a bounded query: MI355REC_BOUNDED_COSINE (0) or MI355REC_BOUNDED_EUCLIDEAN (1)", members=one, metric=-1)
        _refused(nd, "bound nan in a bounded query: a floor is finite", members=one, bound=float("nan"))
        _refused(nd, "bound inf in a bounded query: a floor is finite", members=one, bound=float("inf"))
        _refused(nd, "bound -inf in a bounded query: a radius is finite", members=one, bound=float("-inf"), metric=bo.EUCLIDEAN)
        _refused(nd, "radius -0.5 in a bounded query: a radius is >= 0", members=one, bound=-0.5, metric=bo.EUCLIDEAN)
        _refused(nd, "null out_total in a bounded result", members=one, null_total=True)
        _refused(nd, "null out_idx in a bounded result with topn 5", members=one, topn=5, null_idx=True)
        _refused(nd, "topn -1 out of [0, 1024] (a bounded query has one round; 0 counts only)", members=one, topn=-1)
        _refused(nd, "topn 1025 out of [0, 1024] (a bounded query has one round; 0 counts only)", members=one, topn=1025)
        _refused(nd, "bounded requests take no feature scales", members=one, ext=ext)
        # the shared fields: the playlist request's limits and messages
        _refused(nd, "playlist of 33 songs: 1 to 32 are supported", members=np.zeros((33, 12), np.float32))
        _refused(nd, "Invalid song index: 64", rows=[64])
        _refused(nd, "excluded row 64 out of the catalogue", members=one, exclude=[64])
        _refused(nd, "label 1024 out of [0, 1024)", members=one, labels=[1024])
        _refused(nd, "this handle has no labels (mi355rec_sharded_set_labels)", members=one, labels=[3])
        # structs cut at a field end: the later fields read as zero (metric 0 = cosine, bound 0.0; topn 0 = count only)
        v = bo.values(feats, one, bo.COSINE)
        ok = bo.admissible(feats, v)
        rc, ids, sc, total = bo.request_call(capi, nd._lib.mi355rec_sharded_query_bounded_request, nd._h, members=one, size=64, metric=1, bound=0.9, topn=8)
        assert rc == capi.OK
        bo.check((ids, sc, total), bo.expected_from_values(v, ok, bo.COSINE, 0.0, 8), "cut before metric")
        rc, ids, sc, total = bo.request_call(capi, nd._lib.mi355rec_sharded_query_bounded_request, nd._h, members=one, size=68, metric=0, bound=0.9, topn=8)
        bo.check((ids, sc, total), bo.expected_from_values(v, ok, bo.COSINE, 0.0, 8), "cut before bound")
        # count only with no id buffer at all
        rc, ids, sc, total = bo.request_call(capi, nd._lib.mi355rec_sharded_query_bounded_request, nd._h, members=one, bound=0.9, topn=0, null_idx=True)
        assert rc == capi.OK and total == bo.expected_from_values(v, ok, bo.COSINE, 0.9, 0)[2]
        assert nd._lib.mi355rec_sharded_query_bounded_request(None, None, None, None) == capi.ERR_INVALID_ARG


def test_bindings_and_header(engine_lib):
    from spotify_recommender_amd import capi
    header = (Path(__file__).resolve().parents[1] / "include" / "mi355rec_diag.h").read_text()
    for name in ("mi355rec_query_bounded_request", "mi355rec_sharded_query_bounded_request"):
        assert name in capi.SIGNATURES and re.search(r"\bint " + name + r"\(", header)
        assert getattr(engine_lib, name) is not None
    assert "BOUNDED REQUESTS" in header and "} mi355rec_bounded_query_t;" in header


def test_the_conversion_under_sanitizers(tmp_path):
    """tests/bounded_check.cpp (csrc/playlist_request.h's bounded conversion, floor and cut) built with AddressSanitizer and UBSan and
    run as its own process: nothing is preloaded into python."""
    import subprocess
    root = Path(__file__).resolve().parents[1]
    exe = tmp_path / "bounded_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{root / 'include'}",
           f"-I{root / 'spotify_recommender_amd' / 'csrc'}", str(root / "tests" / "bounded_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and "bounded requests (playlist_request.h): ok" in p.stdout, p.stdout + p.stderr
