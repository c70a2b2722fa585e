"""ANY-OF REQUESTS on a host without a GPU (include/mi355rec_diag.h): mi355rec_sharded_query_anyof_request served by the product's
CPU backend (csrc/cpu_backend.cpp) against tests/anyof_oracle.py — equal ids, bit-equal scores, equal member indices, equal
counts, the padding — plus the identities the contract names, every refusal with its message, the short structs, the bindings
and engine.query_anyof."""
import ctypes

import numpy as np
import pytest

from tests.anyof_oracle import check, expected_from_v, request_call, value
from tests.distance_oracle import hostile_catalogue
from tests.playlist_labels_oracle import uniform_labels


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

SIZES = (1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4097)
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [1, 4, 4, 9]


def _fn(nd):
    return nd._lib.mi355rec_sharded_query_anyof_request


def _ext(capi, rowset, mode):
    return capi.RequestExt(ctypes.sizeof(capi.RequestExt), mode, None, rowset._ptr())


def _call(nd, **kw):
    from spotify_recommender_amd import capi
    rc, ids, sc, mem = request_call(capi, _fn(nd), nd._h, **kw)
    assert rc == capi.OK, nd._lib.mi355rec_sharded_last_error(nd._h)
    return ids, sc, mem


@pytest.mark.parametrize("n", SIZES)
def test_parity(engine_lib, n):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(n)
    lab = uniform_labels(n, 12, 3, unlabelled=0.05)
    rng = np.random.default_rng([11, n])
    in_set = sorted({int(r) for r in rng.choice(n, size=max(1, n // 3), replace=False)})
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(lab)
        with nd.row_set(in_set) as rs:
            for k in (1, 3, 32):
                rows = [int(r) for r in rng.choice(n, size=k, replace=n < k)]
                rows[0] = 0                                              # row 0 has duplicates: ties by row
                vecs = rng.random((k, 12), dtype=np.float32)
                vecs[0] = feats[0]
                for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []),
                                                    ("by row", dict(rows=rows), feats[rows], rows)):
                    v, a = value(feats, members)
                    excl = [0, 0, n // 2, n - 1]
                    for topn in (1, 10, 257, 1024):
                        tag = f"n={n} k={k} {what} top-{topn}"
                        check(_call(nd, topn=topn, **kw), expected_from_v(feats, v, a, excluded, topn), tag)
                        for mode, only in ((capi.ROWSET_EXCLUDE, False), (capi.ROWSET_ONLY, True)):
                            check(_call(nd, topn=topn, exclude=excl, where=WHERE, labels=WANTED, ext=_ext(capi, rs, mode), **kw),
                                  expected_from_v(feats, v, a, excluded + excl, topn, WHERE, lab, WANTED, in_set, only),
                                  tag + f" all together, row set mode {mode}")
                    check(_call(nd, topn=10, exclude=excl, **kw), expected_from_v(feats, v, a, excluded + excl, 10), "exclude")
                    check(_call(nd, topn=10, where=WHERE, **kw), expected_from_v(feats, v, a, excluded, 10, WHERE), "filter")
                    check(_call(nd, topn=10, labels=WANTED, **kw), expected_from_v(feats, v, a, excluded, 10, None, lab, WANTED), "labels")
                    # out_member and out_score are optional: the ids do not depend on them
                    ids = _call(nd, topn=10, want_member=False, want_score=False, **kw)[0]
                    assert ids.tolist() == expected_from_v(feats, v, a, excluded, 10)[0].tolist()


def _merge_one_member(nd, members_kw, k, excluded, topn):
    """The host merge a caller must do today: K one-member playlist requests, the max per row, canonical order, the first N."""
    best = {}
    for m in range(k):
        if "rows" in members_kw:
            ids, sc = nd.query_mean_topn(members_kw["feats"][[members_kw["rows"][m]]], topn, exclude=excluded)
        else:
            ids, sc = nd.query_mean_topn(members_kw["members"][[m]], topn, exclude=excluded)
        for i, s in zip(ids.tolist(), sc.tolist()):
            if i not in best or s > best[i]:
                best[i] = s
    order = sorted(best, key=lambda i: (-best[i], i))[:topn]
    return np.asarray(order, np.int64), np.asarray([best[i] for i in order], np.float32)


def test_identities(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 2049
    feats = hostile_catalogue(n)
    rng = np.random.default_rng(3)
    vecs = rng.random((5, 12), dtype=np.float32)
    rows = [0, 17, 400, 2048, 1023]
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        for topn in (1, 10, 257):
            # K = 1: the playlist request with the same single member, member all 0
            ids, sc, mem = _call(nd, members=vecs[:1], topn=topn, exclude=[5])
            pi, ps = nd.query_mean_topn(vecs[:1], topn, exclude=[5])
            assert ids.tolist() == pi.tolist() and np.array_equal(sc.view(np.uint32), ps.view(np.uint32)) and not mem.any()
            ids, sc, mem = _call(nd, rows=rows[:1], topn=topn)
            pi, ps = nd.query_playlist_topn(rows[:1], topn)
            assert ids.tolist() == pi.tolist() and np.array_equal(sc.view(np.uint32), ps.view(np.uint32)) and not mem.any()
            # a duplicated member changes nothing; the member index names the first occurrence
            base = _call(nd, members=vecs, topn=topn)
            dup = _call(nd, members=np.concatenate([vecs, vecs[1:3]]), topn=topn)
            check(dup, base, "duplicate members")
            # permuted members: the same ids and score bits; the member named attains the maximum
            perm = np.asarray([3, 0, 4, 2, 1])
            pid, psc, pmem = _call(nd, members=vecs[perm], topn=topn)
            assert pid.tolist() == base[0].tolist() and np.array_equal(psc.view(np.uint32), base[1].view(np.uint32))
            from tests.anyof_oracle import member_scores
            c = member_scores(feats, vecs[perm])
            assert np.array_equal((c[pmem, pid] + np.float32(0)).view(np.uint32), psc.view(np.uint32))
            # the union of K one-member answers, each with the whole exclusion list and the member rows
            ui, us = _merge_one_member(nd, dict(members=vecs), 5, [5, 9], topn)
            ids, sc, _ = _call(nd, members=vecs, topn=topn, exclude=[5, 9])
            assert ids.tolist() == ui.tolist() and np.array_equal(sc.view(np.uint32), us.view(np.uint32))
            ui, us = _merge_one_member(nd, dict(rows=rows, feats=feats), 5, [5, 9] + rows, topn)
            ids, sc, _ = _call(nd, rows=rows, topn=topn, exclude=[5, 9])
            assert ids.tolist() == ui.tolist() and np.array_equal(sc.view(np.uint32), us.view(np.uint32))


def test_zero_norm_and_tiny_members(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 300
    feats = hostile_catalogue(n)
    rng = np.random.default_rng(4)
    vecs = rng.random((4, 12), dtype=np.float32)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        for bad in (0.0, 1e-30, 1e-10, 1e30, np.nan, np.inf):
            m = vecs.copy()
            m[1] = np.float32(bad)
            v, a = value(feats, m)
            check(_call(nd, members=m, topn=50), expected_from_v(feats, v, a, [], 50), f"member of {bad}")
            z = np.full((2, 12), np.float32(bad))
            v, a = value(feats, z)
            check(_call(nd, members=z, topn=50), expected_from_v(feats, v, a, [], 50), f"all members {bad}")


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
            refused("in an any-of query: must be 0", members=v, flags=flags)
        refused("members by value and by row in one any-of query", members=v, rows=[1, 2])
        refused("an any-of query needs members by value or by row", topn=10)
        full = ctypes.sizeof(capi.AnyOfQuery)
        assert full == 64
        for size in (0, 2, 6, 12, 47, 50, 63, full + 1, full + 8, 88):
            refused(f"any-of query of size {size}: not the end of a field", members=v, size=size)
        refused("has no labels", members=v, labels=[1])
        nd.set_labels(np.zeros(300, np.int32))
        refused("n_labels must be positive", members=v, labels=[])
        refused("n_labels must be positive", members=v, labels=[1], n_labels=-1)
        refused("null label set", members=v, n_labels=2)
        refused("label 1024 out of", members=v, labels=[3, 1024])
        refused("label -1 out of", members=v, labels=[-1])
        for k in (0, -1, 33):
            refused(f"playlist of {k} songs", members=np.zeros((40, 12), np.float32), k=k)
        for topn in (0, -3, 1025):
            refused(f"topn {topn} out of [1, 1024]", members=v, topn=topn)
        refused("n_exclude -1 out of", members=v, n_exclude=-1)
        refused("n_exclude 1025 out of", members=v, exclude=list(range(300)) * 4, n_exclude=1025)
        refused("null exclusion list with n_exclude 3", members=v, n_exclude=3)
        refused("excluded row 300 out of the catalogue", members=v, exclude=[300])
        refused("excluded row -1 out of the catalogue", members=v, exclude=[-1])
        refused("Invalid song index: 300", rows=[1, 300])
        refused("Invalid song index: -1", rows=[-1])
        # the ext: feature scales refused, a row set of another handle, a bad mode, a bad size
        ones = np.ones(12, np.float32)
        refused("any-of requests take no feature scales", members=v,
                ext=capi.RequestExt(ctypes.sizeof(capi.RequestExt), 0, ones.ctypes.data_as(ctypes.c_void_p), None))
        with other.row_set([1, 2]) as foreign, nd.row_set([1, 2]) as mine:
            refused("row set of another handle", members=v, ext=_ext(capi, foreign, capi.ROWSET_ONLY))
            refused("rowset_mode 2", members=v, ext=capi.RequestExt(ctypes.sizeof(capi.RequestExt), 2, None, mine._ptr()))
            refused("request ext of size 5", members=v, ext=capi.RequestExt(5, 0, None, mine._ptr()))
            # a short query struct that ends where a field ends is read as "later fields zero": topn 0 is then refused as topn
            refused("topn 0 out of", members=v, size=capi.AnyOfQuery.topn.offset)
        bad = capi.Filter()
        bad.active = 1 << 12
        q = capi.AnyOfQuery(size=full, members=v.ctypes.data_as(ctypes.c_void_p), k=2, topn=5, filter=ctypes.pointer(bad))
        idx = np.zeros(5, np.int64)
        res = capi.AnyOfResult(idx.ctypes.data_as(ctypes.c_void_p), None, None, None)
        assert _fn(nd)(nd._h, ctypes.byref(q), None, ctypes.byref(res)) == capi.ERR_INVALID_ARG
        # null structs, a null out_idx; out_score, out_member and out_count may be null
        assert _fn(nd)(nd._h, None, None, ctypes.byref(res)) == capi.ERR_INVALID_ARG
        assert _fn(nd)(nd._h, ctypes.byref(q), None, None) == capi.ERR_INVALID_ARG
        q.filter = None
        assert _fn(nd)(nd._h, ctypes.byref(q), None, ctypes.byref(capi.AnyOfResult(None, None, None, None))) == capi.ERR_INVALID_ARG
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
        v, a = value(feats, feats[rows])
        check(engine.query_anyof(nd, 20, rows=rows), expected_from_v(feats, v, a, rows, 20), "rows")
        check(engine.query_anyof(nd, 20, rows=rows, exclude=[1, 2], where=WHERE, labels=WANTED, seen=seen),
              expected_from_v(feats, v, a, rows + [1, 2], 20, WHERE, lab, WANTED, seen, False), "rows, everything, seen")
        v, a = value(feats, vecs)
        check(engine.query_anyof(nd, 20, members=vecs, only=seen), expected_from_v(feats, v, a, [], 20, rowset=seen, rowset_only=True), "only")
        with pytest.raises(ValueError):
            engine.query_anyof(nd, 5)
        with pytest.raises(ValueError):
            engine.query_anyof(nd, 5, members=vecs, rows=rows)
        with pytest.raises(ValueError):
            engine.query_anyof(nd, 5, members=vecs, seen=seen, only=seen)
