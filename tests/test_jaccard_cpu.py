"""JACCARD REQUESTS on a host without a GPU (include/mi355rec_diag.h): mi355rec_sharded_query_jaccard_request served by the
product's CPU backend (csrc/cpu_backend.cpp) through the node handle against tests/jaccard_oracle.py — equal ids, bit-equal
similarities, equal counts, the padding — the chain against float64, a copy of the single member at exactly 1.0f, the rows that
form no key, every refusal with its message, the short structs, the bindings, engine.query_jaccard and
Recommender::Query::jaccard.  (The CLI: tests/test_jaccard_cli.py.)"""
import ctypes

import numpy as np
import pytest

from tests.jaccard_oracle import check, cross_check, expected_from_v, hostile_catalogue, mean_jaccard, request_call
from tests.playlist_labels_oracle import uniform_labels
from tests.test_rowset_cli import Shim, catalogue, golden  # noqa: F401  (catalogue, golden: the fixtures)


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

SIZES = (1, 5, 257, 4097)
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [1, 4, 4, 9]
ONE = np.float32(1.0).view(np.uint32)


def _fn(nd):
    return nd._lib.mi355rec_sharded_query_jaccard_request


def _ext(capi, rowset, mode):
    return capi.RequestExt(ctypes.sizeof(capi.RequestExt), mode, None, rowset._ptr())


def _call(nd, **kw):
    from spotify_recommender_amd import capi
    rc, ids, sim = request_call(capi, _fn(nd), nd._h, **kw)
    assert rc == capi.OK, nd._lib.mi355rec_sharded_last_error(nd._h)
    return ids, sim


@pytest.mark.parametrize("n", SIZES)
def test_parity(engine_lib, n):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(n)
    lab = uniform_labels(n, 12, 3, unlabelled=0.05)
    rng = np.random.default_rng([29, n])
    in_set = sorted({int(r) for r in rng.choice(n, size=max(1, n // 3), replace=False)})
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(lab)
        with nd.row_set(in_set) as rs:
            for k in (1, 3, 32):
                rows = [int(r) for r in rng.choice(n, size=k, replace=n < k)]
                rows[0] = 0                                              # row 0 has duplicates: v = 1 and ties by row
                vecs = rng.random((k, 12), dtype=np.float32)
                vecs[0] = feats[0]
                for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []),
                                                    ("by row", dict(rows=rows), feats[rows], rows)):
                    vv = mean_jaccard(feats, members)
                    cross_check(feats, members, *vv)
                    excl = [0, 0, n // 2, n - 1]
                    for topn in (1, 10, 1024):
                        tag = f"n={n} k={k} {what} top-{topn}"
                        check(_call(nd, topn=topn, **kw), expected_from_v(feats, vv, excluded, topn), tag)
                        for mode, only in ((capi.ROWSET_EXCLUDE, False), (capi.ROWSET_ONLY, True)):
                            check(_call(nd, topn=topn, exclude=excl, where=WHERE, labels=WANTED, ext=_ext(capi, rs, mode), **kw),
                                  expected_from_v(feats, vv, excluded + excl, topn, WHERE, lab, WANTED, in_set, only),
                                  tag + f" all together, row set mode {mode}")
                    check(_call(nd, topn=10, exclude=excl, **kw), expected_from_v(feats, vv, excluded + excl, 10), "exclude")
                    check(_call(nd, topn=10, where=WHERE, **kw), expected_from_v(feats, vv, excluded, 10, WHERE), "filter")
                    check(_call(nd, topn=10, labels=WANTED, **kw), expected_from_v(feats, vv, excluded, 10, None, lab, WANTED), "labels")
                    # out_similarity is optional: the ids do not depend on it
                    ids = _call(nd, topn=10, want_similarity=False, **kw)[0]
                    assert ids.tolist() == expected_from_v(feats, vv, excluded, 10)[0].tolist()


def test_a_copy_scores_exactly_one_ties_go_by_row_and_hostile_rows_form_no_key(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 257
    feats = hostile_catalogue(n)                                         # rows 8, 9, 10, n // 2 and n - 1 are copies of row 0
    copies = [0, 8, 9, 10, n // 2, n - 1]
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        ids, sim = _call(nd, members=feats[:1], topn=8)
        assert ids[:6].tolist() == copies and np.all(sim[:6].view(np.uint32) == ONE) and sim[6] < 1
        vv = mean_jaccard(feats, feats[:1])
        check((ids, sim), expected_from_v(feats, vv, [], 8), "copies of the member")
        # NaN, +inf and -inf rows form no key: the count says so; the formula is applied as written to the negative of the member (-1)
        ids, sim = _call(nd, members=feats[:1], topn=1024)
        assert ids.size == int(vv[1].sum()) == n - 3 and np.all(np.isfinite(sim)) and not {2, 3, 4} & set(ids.tolist())
        assert sim[ids.tolist().index(12)] == -1.0
        # an all-zero member: the all-zero row is 0 / 0, the all-negative row -x / 0: neither is ever returned
        zero = np.zeros((1, 12), np.float32)
        ids, sim = _call(nd, members=zero, topn=1024)
        assert not {5, 13} & set(ids.tolist())
        check((ids, sim), expected_from_v(feats, mean_jaccard(feats, zero), [], 1024), "the all-zero member")
        for bad in (np.nan, np.inf, -np.inf, 1e30, 1e-30, 0.0, -0.5):
            members = np.vstack([feats[1], np.full(12, bad, np.float32)])
            check(_call(nd, members=members, topn=300), expected_from_v(feats, mean_jaccard(feats, members), [], 300), f"a member of {bad}")
        one_nan = feats[1:2].copy()
        one_nan[0, 7] = np.nan                                           # a NaN in a member reaches num: no row forms a key
        assert _call(nd, members=one_nan, topn=50)[0].size == 0 and not mean_jaccard(feats, one_nan)[1].any()


def test_refusals(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(300)
    v = feats[:2]
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd, NodeEngine(feats[:50], placement=capi.PLACEMENT_AUTO) as other:
        def refused(msg, **kw):
            rc = request_call(capi, _fn(nd), nd._h, **kw)[0]
            text = nd._lib.mi355rec_sharded_last_error(nd._h).decode()
            assert rc == capi.ERR_INVALID_ARG and msg in text, (sorted(kw), rc, text)

        for flags in (1, 2, 4, 8, 0x80000000):
            refused("in a jaccard query: must be 0", members=v, flags=flags)
        refused("members by value and by row in one jaccard query", members=v, rows=[1, 2])
        refused("a jaccard query needs members by value or by row", topn=10)
        full = ctypes.sizeof(capi.JaccardQuery)
        assert full == 64
        for size in (0, 2, 6, 12, 47, 50, 63, full + 1, full + 8, 88):
            refused(f"jaccard query of size {size}: not the end of a field", members=v, size=size)
        refused("has no labels", members=v, labels=[1])
        nd.set_labels(np.zeros(300, np.int32))
        refused("n_labels must be positive", members=v, labels=[])
        refused("null label set", members=v, n_labels=2)
        refused("label 1024 out of", members=v, labels=[3, 1024])
        for k in (0, -1, 33):
            refused(f"playlist of {k} songs", members=np.zeros((40, 12), np.float32), k=k)
        for topn in (0, -3, 1025):
            refused(f"topn {topn} out of [1, 1024]", members=v, topn=topn)
        refused("n_exclude -1 out of", members=v, n_exclude=-1)
        refused("null exclusion list with n_exclude 3", members=v, n_exclude=3)
        refused("excluded row 300 out of the catalogue", members=v, exclude=[300])
        refused("Invalid song index: 300", rows=[1, 300])
        refused("Invalid song index: -1", rows=[-1])
        # the ext: feature scales refused, a row set of another handle, a bad mode, a bad size
        ones = np.ones(12, np.float32)
        refused("jaccard requests take no feature scales", members=v,
                ext=capi.RequestExt(ctypes.sizeof(capi.RequestExt), 0, ones.ctypes.data_as(ctypes.c_void_p), None))
        with other.row_set([1, 2]) as foreign, nd.row_set([1, 2]) as mine:
            refused("row set of another handle", members=v, ext=_ext(capi, foreign, capi.ROWSET_ONLY))
            refused("rowset_mode 2", members=v, ext=capi.RequestExt(ctypes.sizeof(capi.RequestExt), 2, None, mine._ptr()))
            refused("request ext of size 5", members=v, ext=capi.RequestExt(5, 0, None, mine._ptr()))
            # a short query struct that ends where a field ends is read as "later fields zero": topn 0 is then refused as topn
            refused("topn 0 out of", members=v, size=capi.JaccardQuery.topn.offset)
        q = capi.JaccardQuery(size=full, members=v.ctypes.data_as(ctypes.c_void_p), k=2, topn=5)
        idx = np.zeros(5, np.int64)
        res = capi.JaccardResult(idx.ctypes.data_as(ctypes.c_void_p), None, None)
        # null structs, a null out_idx, a null handle; out_similarity and out_count may be null
        assert _fn(nd)(nd._h, None, None, ctypes.byref(res)) == capi.ERR_INVALID_ARG
        assert _fn(nd)(nd._h, ctypes.byref(q), None, None) == capi.ERR_INVALID_ARG
        assert _fn(nd)(nd._h, ctypes.byref(q), None, ctypes.byref(capi.JaccardResult(None, None, None))) == capi.ERR_INVALID_ARG
        assert _fn(nd)(nd._h, ctypes.byref(q), None, ctypes.byref(res)) == capi.OK
        assert idx.tolist() == _call(nd, members=v, topn=5)[0].tolist()
        assert _fn(nd)(None, ctypes.byref(q), None, ctypes.byref(res)) == capi.ERR_INVALID_ARG


def test_python_function(engine_lib):
    from spotify_recommender_amd import capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 777
    feats = hostile_catalogue(n)
    lab = uniform_labels(n, 12, 3, unlabelled=0.05)
    rows = [0, 300, 776]
    vecs = np.random.default_rng(8).random((3, 12), dtype=np.float32)
    seen = list(range(10, 200, 3))
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        nd.set_labels(lab)
        vv = mean_jaccard(feats, feats[rows])
        check(engine.query_jaccard(nd, 20, rows=rows), expected_from_v(feats, vv, rows, 20), "rows")
        check(engine.query_jaccard(nd, 20, rows=rows, exclude=[1, 2], where=WHERE, labels=WANTED, seen=seen),
              expected_from_v(feats, vv, rows + [1, 2], 20, WHERE, lab, WANTED, seen, False), "rows, everything, seen")
        vv = mean_jaccard(feats, vecs)
        check(engine.query_jaccard(nd, 20, members=vecs, only=seen), expected_from_v(feats, vv, [], 20, rowset=seen, rowset_only=True), "only")
        with pytest.raises(ValueError):
            engine.query_jaccard(nd, 5)
        with pytest.raises(ValueError):
            engine.query_jaccard(nd, 5, members=vecs, rows=rows)
        with pytest.raises(ValueError):
            engine.query_jaccard(nd, 5, members=vecs, seen=seen, only=seen)


# ---- the C++ class ----------------------------------------------------------------------------------------------------------
def features_of(shim):
    fn = shim.L.shim_song_features
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    out = np.zeros((shim.n, 12), np.float32)
    genre = ctypes.c_int(0)
    for i in range(shim.n):
        assert fn(shim.h, i, out[i].ctypes.data, ctypes.byref(genre)) == 1
    return out


def _jaccard(shim, songs, topn, exclude=(), where=None, refuse=0):
    fn = shim.L.shim_query_jaccard
    fn.restype = ctypes.c_int64
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fn.argtypes = [P, P, I, P, I, I, F, F, I, I, P, P, ctypes.c_int64]
    s, ex = np.asarray(songs, np.int32), np.asarray(list(exclude) or [0], np.int32)
    out, sc = np.full(1024, -7, np.int32), np.zeros(1024, np.float32)
    f, lo, hi = where if where is not None else (-1, 0.0, 0.0)
    n = fn(shim.h, s.ctypes.data, len(songs), ex.ctypes.data, len(exclude), f, lo, hi, topn, refuse, out.ctypes.data, sc.ctypes.data, 1024)
    assert n >= 0
    return out[:n].astype(np.int64), sc[:n].copy()


def test_recommender_jaccard(catalogue):  # noqa: F811
    shim, _ = catalogue
    feats = features_of(shim)
    members = [5, 70, 333]
    vv = mean_jaccard(feats, feats[members])
    for topn in (1, 10, 100):
        check(_jaccard(shim, members, topn), expected_from_v(feats, vv, members, topn), f"top-{topn}")
        check(_jaccard(shim, members, topn, exclude=[1, 2, 3], where=(1, 0.2, 0.9)),
              expected_from_v(feats, vv, members + [1, 2, 3], topn, {1: (0.2, 0.9)}), f"top-{topn}, exclusion and range")
    seen = list(range(0, shim.n, 3))
    assert shim.set_rows(seen) == 1                               # the row set of setRowSet applies
    check(_jaccard(shim, members, 20), expected_from_v(feats, vv, members, 20, rowset=seen), "row set")
    shim.clear()
    for bit in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):     # refused with a message and {}
        assert _jaccard(shim, members, 10, refuse=bit)[0].size == 0, bit
    check(_jaccard(shim, members, 10), expected_from_v(feats, vv, members, 10), "after the refusals")
