"""ROW SETS on a host without a GPU (include/mi355rec_diag.h): the node-handle _ext entry points served by the product's CPU backend
against tests/rowset_oracle.py (the existing oracles with exclude + S, or exclude + the complement of S) — equal ids, bit-equal
scores and distances, counts and padding — every identity of the header, every refusal with its message, the struct's layout and
size rules, the Python `seen=` / `only=` forms, and csrc/rowset.h itself: its slice function against numpy and a stand-alone
program (tests/rowset_check.cpp) under AddressSanitizer and UBSan, run as its own process."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import distance_oracle, playlist_labels_oracle, rowset_oracle
from tests.playlist_labels_oracle import uniform_labels
from tests.rowset_oracle import EXCLUDE, MODES, ONLY, excluded, prefix, request_call, shapes
from tests.scaled_oracle import GENERAL, cosine_expected, cosine_scores, distance_expected, distance_m

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "spotify_recommender_amd" / "csrc"


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 9, 33, 257, 2049]
TOPNS = (1, 10, 1024)
METRICS = ("cosine", "euclidean")
FN = {"cosine": "mi355rec_sharded_query_playlist_request_ext", "euclidean": "mi355rec_sharded_query_distance_request_ext"}
ONES = np.ones(12, np.float32)


def _node(feats):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(feats, placement=capi.PLACEMENT_AUTO)
    assert nd.placement() == capi.PLACEMENT_CPU
    return nd


def _err(nd):
    return nd._lib.mi355rec_sharded_last_error(nd._h).decode()


def _call(nd, metric, rowset, mode, **kw):
    from spotify_recommender_amd import capi
    got = request_call(capi, getattr(nd._lib, FN[metric]), nd._h, metric, rowset._ptr() if rowset is not None else None, mode, **kw)
    assert got[0] == capi.OK, _err(nd)
    return got[1], got[2]


def _values(metric, feats, members, a=ONES, weights=None):
    return distance_m(feats, members, a) if metric == "euclidean" else cosine_scores(feats, members, a, weights)


def _expected(metric, values, feats, gone, topn, where=None, labels=None, wanted=None):
    fn = distance_expected if metric == "euclidean" else cosine_expected
    return fn(values, feats, gone, topn, where, labels, wanted)


def _feats(n):
    from oracle import oracle
    feats = oracle.mt19937_uniform(700 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    return feats


@cpu_only
@pytest.mark.parametrize("n", SIZES)
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
                v_w = _values(metric, feats, vecs, weights=signed) if metric == "cosine" else None
                sets = shapes(n)
                sets["own_top"] = _expected(metric, v_v, feats, [], min(n, 310))[0]   # the set-less request's own best rows
                for sname, ids in sets.items():
                    with nd.row_set(np.concatenate([ids, ids[:3]])) as s:       # (duplicates are allowed)
                        assert s.count == ids.size
                        for mname, mode in MODES:
                            what = f"n={n} K={k} {metric} {sname} {mname}"
                            gone = excluded(n, ids, mode)
                            want_r = _expected(metric, v_r, feats, np.concatenate([rows, gone]), 1024)
                            want_v = _expected(metric, v_v, feats, gone, 1024)
                            assert want_v[0].size == min(1024, rowset_oracle.admitted(n, ids, mode)) or metric == "euclidean"
                            for topn in TOPNS:
                                distance_oracle.check(_call(nd, metric, s, mode, rows=rows, topn=topn), prefix(want_r, topn), what + " by row")
                                distance_oracle.check(_call(nd, metric, s, mode, members=vecs, topn=topn), prefix(want_v, topn), what + " by value")
                            ex = [n - 1, 0, 0]
                            distance_oracle.check(_call(nd, metric, s, mode, members=vecs, exclude=ex, where=WHERE, labels=WANTED, topn=10),
                                                  _expected(metric, v_v, feats, excluded(n, ids, mode, ex), 10, WHERE, lab, WANTED),
                                                  what + " composed")
                            if metric == "cosine":
                                distance_oracle.check(_call(nd, metric, s, mode, members=vecs, weights=signed, exclude=[0], where=WHERE, topn=10),
                                                      _expected(metric, v_w, feats, excluded(n, ids, mode, [0]), 10, WHERE), what + " signed")
                            distance_oracle.check(_call(nd, metric, s, mode, members=vecs, scales=GENERAL, topn=10),
                                                  _expected(metric, _values(metric, feats, vecs, GENERAL), feats, gone, 10), what + " scaled")


@cpu_only
@pytest.mark.parametrize("n", [33, 257, 2049])
def test_prior_diverse_and_capped_get_the_admissible_pool(engine_lib, n):
    from spotify_recommender_amd import capi
    from tests import prior_oracle
    feats = _feats(n)
    rng = np.random.default_rng([4, n])
    groups = rng.integers(-1, 12, size=n).astype(np.int32)
    priors = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    vecs = rng.random((3, 12), dtype=np.float32)
    sc = playlist_labels_oracle.scores_of(feats, vecs)
    fn = getattr(capi.lib(), FN["cosine"])
    with _node(feats) as nd:
        nd.set_groups(groups)
        nd.set_priors(priors)
        for sname, ids in shapes(n).items():
            with nd.row_set(ids) as s:
                for mname, mode in MODES:
                    what = f"n={n} {sname} {mname}"
                    gone = excluded(n, ids, mode, [1])
                    rc, gi, gs, _, _ = request_call(capi, fn, nd._h, "cosine", s._ptr(), mode, members=vecs, exclude=[1], topn=10, prior_weight=0.75)
                    assert rc == capi.OK, _err(nd)
                    distance_oracle.check((gi, gs), prior_oracle.expected_prior(sc, priors, 0.75, feats, None, None, gone, 10), what + " prior")
                    for topn, pool in ((5, 5), (10, 40)):
                        pool_rows = playlist_labels_oracle.expected_scored(sc, feats, None, None, gone, pool)
                        rc, gi, gs, gm, _ = request_call(capi, fn, nd._h, "cosine", s._ptr(), mode, members=vecs, exclude=[1], topn=topn,
                                                         lam=0.6, pool=pool)
                        assert rc == capi.OK, _err(nd)
                        wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, topn)
                        distance_oracle.check((gi, gs), (wi, ws), what + f" diverse top-{topn} of {pool}")
                        assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), what + " mmr"
                        rc, gi, gs, gm, p_rows = request_call(capi, fn, nd._h, "cosine", s._ptr(), mode, members=vecs, exclude=[1], topn=topn,
                                                              lam=0.6, pool=pool, max_per_group=2)
                        assert rc == capi.OK, _err(nd)
                        wi, ws, wm = playlist_labels_oracle.expected_diverse(pool_rows, feats, 0.6, topn, groups, 2)
                        distance_oracle.check((gi, gs), (wi, ws), what + f" capped top-{topn} of {pool}")
                        assert p_rows == pool_rows[0].size


@cpu_only
def test_identities(engine_lib):
    from spotify_recommender_amd import capi
    n = 2049
    feats = _feats(n)
    rng = np.random.default_rng(8)
    vecs = rng.random((3, 12), dtype=np.float32)
    small = rng.choice(n, size=700, replace=False).astype(np.int64)
    plain = {"cosine": ("mi355rec_sharded_query_playlist_request", playlist_labels_oracle.request_call),
             "euclidean": ("mi355rec_sharded_query_distance_request", distance_oracle.request_call)}
    scaled = {"cosine": "mi355rec_sharded_query_playlist_request_scaled", "euclidean": "mi355rec_sharded_query_distance_request_scaled"}
    with _node(feats) as nd, nd.row_set(small) as s, nd.row_set([]) as empty, nd.row_set(np.arange(n)) as full:
        assert (s.count, empty.count, full.count) == (700, 0, n)
        for metric in METRICS:
            name, req = plain[metric]
            for kw in (dict(rows=[5, 9]), dict(members=vecs, exclude=[1, 2], where=WHERE)):
                want = req(capi, getattr(nd._lib, name), nd._h, topn=100, **kw)[1:3]
                fn = getattr(nd._lib, FN[metric])
                for what, got in (("NULL ext", request_call(capi, fn, nd._h, metric, None, 0, ext_null=True, topn=100, **kw)),
                                  ("two NULL pointers", request_call(capi, fn, nd._h, metric, None, 7, topn=100, **kw)),
                                  ("EXCLUDE, empty set", request_call(capi, fn, nd._h, metric, empty._ptr(), EXCLUDE, topn=100, **kw)),
                                  ("ONLY, every row", request_call(capi, fn, nd._h, metric, full._ptr(), ONLY, topn=100, **kw))):
                    assert got[0] == capi.OK, _err(nd)
                    distance_oracle.check(got[1:3], want, f"{metric} {what}")
                for what, rowset, mode in (("ONLY, empty set", empty, ONLY), ("EXCLUDE, every row", full, EXCLUDE)):
                    got = request_call(capi, fn, nd._h, metric, rowset._ptr(), mode, topn=100, **kw)
                    assert got[0] == capi.OK and got[1].size == 0, what
                # scales only: the _scaled call
                def with_scales(handle, query, result, metric=metric):
                    return getattr(nd._lib, scaled[metric])(handle, query, GENERAL.ctypes.data_as(ctypes.c_void_p), result)
                kw_s = {key: v for key, v in kw.items()}
                want_s = req(capi, with_scales, nd._h, topn=100, **kw_s)[1:3]
                got = request_call(capi, fn, nd._h, metric, None, 0, scales=GENERAL, topn=100, **kw)
                assert got[0] == capi.OK, _err(nd)
                distance_oracle.check(got[1:3], want_s, f"{metric} scales only")
                # EXCLUDE with |S| <= 1024: the request with S appended to exclude_global
                ex = list(kw.get("exclude", [])) + small.tolist()
                kw_x = dict(kw, exclude=ex)
                want_x = req(capi, getattr(nd._lib, name), nd._h, topn=100, **kw_x)[1:3]
                got = request_call(capi, fn, nd._h, metric, s._ptr(), EXCLUDE, topn=100, **kw)
                assert got[0] == capi.OK, _err(nd)
                distance_oracle.check(got[1:3], want_x, f"{metric} S appended to exclude_global")


@cpu_only
def test_add_and_count(engine_lib):
    n = 2049
    feats = _feats(n)
    rng = np.random.default_rng(12)
    ids = rng.choice(n, size=900, replace=False).astype(np.int64)
    vecs = rng.random((2, 12), dtype=np.float32)
    with _node(feats) as nd, nd.row_set(ids) as whole, nd.row_set(ids[:450]) as grown:
        assert grown.count == 450
        grown.add(np.concatenate([ids[400:], ids[:10], ids[-5:]]))      # the rest, with duplicates
        assert grown.count == whole.count == 900
        grown.add([])
        assert grown.count == 900
        for mname, mode in MODES:
            for metric in METRICS:
                distance_oracle.check(_call(nd, metric, grown, mode, members=vecs, topn=100), _call(nd, metric, whole, mode, members=vecs, topn=100),
                                      f"{metric} {mname}: grown against whole")
        # the Python forms: a RowSet, a plain id sequence (a temporary set), and an engine that closes the sets it still has
        a = nd.query_mean_topn(vecs, 20, seen=whole)
        distance_oracle.check(nd.query_mean_topn(vecs, 20, seen=ids.tolist()), a, "seen= as a list")
        distance_oracle.check(nd.query_mean_topn(vecs, 20, exclude=ids[:1024].tolist()), a, "seen= against exclude=")
        comp = np.setdiff1d(np.arange(n), ids)
        distance_oracle.check(nd.query_mean_topn(vecs, 20, only=comp), a, "only= the complement")
        distance_oracle.check(nd.query_playlist_topn([3, 4], 20, only=comp), nd.query_playlist_topn([3, 4], 20, seen=whole), "by row")
        distance_oracle.check(nd.query_nearest_scaled(vecs, 20, None, only=comp), nd.query_nearest(vecs, 20, exclude=ids[:1024].tolist()), "nearest")
        distance_oracle.check(nd.query_nearest_rows_scaled([3, 4], 20, GENERAL, seen=whole),
                              nd.query_nearest_rows_scaled([3, 4], 20, GENERAL, exclude=ids[:1024].tolist()), "nearest rows, scaled")
        d = nd.query_mean_topn_diverse(vecs, 10, 0.5, seen=whole, return_mmr=True)
        e = nd.query_mean_topn_diverse(vecs, 10, 0.5, exclude=ids[:1024].tolist(), return_mmr=True)
        assert all(np.array_equal(x, y) for x, y in zip(d, e))
        nd.set_groups(np.arange(n, dtype=np.int32) % 7)
        d = nd.query_playlist_topn_capped([3, 4], 10, 1, only=comp)
        e = nd.query_playlist_topn_capped([3, 4], 10, 1, exclude=ids[:1024].tolist())
        assert all(np.array_equal(x, y) for x, y in zip(d, e))
        with pytest.raises(ValueError, match="mutually exclusive"):
            nd.query_mean_topn(vecs, 20, seen=whole, only=whole)
        with pytest.raises(ValueError, match="mutually exclusive"):
            nd.query_nearest_scaled(vecs, 20, None, seen=[1], only=[2])
        left = nd.row_set([1, 2, 3])
    assert not left._p and not whole._p            # closed by the engine, and by its own context
    with pytest.raises(ValueError, match="closed"):
        left.count


@cpu_only
def test_refusals(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 257
    feats = _feats(n)
    vecs = feats[:2]
    L = capi.lib()
    with _node(feats) as nd, _node(feats[:100]) as other:
        out = ctypes.c_void_p()

        def create(ids, n_ids):
            a = None if ids is None else np.asarray(ids, np.int64)
            return L.mi355rec_sharded_rowset_create(nd._h, None if a is None else a.ctypes.data_as(ctypes.c_void_p), n_ids, ctypes.byref(out))

        for ids, n_ids, msg in (([3, -1], 2, "row set: id -1 out of [0, 257)"), ([257], 1, "row set: id 257 out of [0, 257)"),
                                ([1], -1, "row set: n_ids must not be negative, got -1"), (None, 2, "row set: null id list with n_ids 2")):
            assert create(ids, n_ids) == capi.ERR_INVALID_ARG and not out.value
            assert _err(nd) == msg
        assert create(None, 0) == capi.OK and out.value                       # n_ids == 0: an empty set
        assert L.mi355rec_rowset_count(out) == 0
        L.mi355rec_rowset_destroy(out)
        L.mi355rec_rowset_destroy(None)                                       # NULL is fine
        assert L.mi355rec_sharded_rowset_create(None, None, 0, ctypes.byref(out)) == capi.ERR_INVALID_ARG
        with nd.row_set([1, 2, 3]) as s, other.row_set([1]) as foreign:
            # a failed add leaves the set unchanged; its message is the global one
            bad = np.asarray([7, 8, 300], np.int64)
            assert L.mi355rec_rowset_add(s._ptr(), bad.ctypes.data_as(ctypes.c_void_p), 3) == capi.ERR_INVALID_ARG
            assert L.mi355rec_last_global_error().decode() == "row set: id 300 out of [0, 257)"
            assert s.count == 3
            assert L.mi355rec_rowset_add(s._ptr(), None, 1) == capi.ERR_INVALID_ARG
            assert L.mi355rec_rowset_add(None, None, 0) == capi.ERR_INVALID_ARG
            with pytest.raises(capi.Mi355Error, match="id -4"):
                s.add([5, -4])
            assert s.count == 3
            for metric in METRICS:
                fn = getattr(L, FN[metric])
                for kw, msg in ((dict(rowset=s._ptr(), mode=2), "rowset_mode 2"), (dict(rowset=foreign._ptr(), mode=0), "row set of another handle"),
                                (dict(rowset=s._ptr(), mode=0, ext_size=0), "request ext of size 0"),
                                (dict(rowset=s._ptr(), mode=0, ext_size=12), "request ext of size 12"),
                                (dict(rowset=s._ptr(), mode=0, ext_size=32), "request ext of size 32"),
                                (dict(rowset=s._ptr(), mode=0, scales=np.full(12, np.nan, np.float32)), "feature scale 0 is nan")):
                    rowset, mode = kw.pop("rowset"), kw.pop("mode")
                    rc = request_call(capi, fn, nd._h, metric, rowset, mode, members=vecs, topn=5, **kw)[0]
                    assert rc == capi.ERR_INVALID_ARG and msg in _err(nd), (metric, msg, _err(nd))
            rc = request_call(capi, getattr(L, FN["cosine"]), nd._h, "cosine", s._ptr(), 0, scales=GENERAL, members=vecs, topn=5, lam=0.5, pool=5)[0]
            assert rc == capi.ERR_INVALID_ARG and "MI355REC_PQ_DIVERSE with feature scales" in _err(nd)
            # the size rules: a shorter struct that ends where a field ends is read as "later fields zero"
            want = request_call(capi, getattr(L, FN["cosine"]), nd._h, "cosine", None, 0, ext_null=True, members=vecs, topn=20)
            for size in (4, 8):                                               # neither scales nor set are read
                got = request_call(capi, getattr(L, FN["cosine"]), nd._h, "cosine", s._ptr(), 2, scales=GENERAL, ext_size=size, members=vecs, topn=20)
                assert got[0] == capi.OK, _err(nd)
                distance_oracle.check(got[1:3], want[1:3], f"ext of size {size}")
            got = request_call(capi, getattr(L, FN["cosine"]), nd._h, "cosine", s._ptr(), 2, scales=GENERAL, ext_size=16, members=vecs, topn=20)
            assert got[0] == capi.OK, _err(nd)                                # the scales are read, the set (and its mode) is not
            distance_oracle.check(got[1:3], request_call(capi, getattr(L, FN["cosine"]), nd._h, "cosine", None, 0, scales=GENERAL, members=vecs, topn=20)[1:3],
                                  "ext of size 16")
    assert isinstance(nd, NodeEngine)


def test_struct_layout(engine_lib):
    from spotify_recommender_amd import capi
    E = capi.RequestExt
    assert ctypes.sizeof(E) == 24
    assert (E.size.offset, E.rowset_mode.offset, E.feature_scales.offset, E.rowset.offset) == (0, 4, 8, 16)
    assert (capi.ROWSET_EXCLUDE, capi.ROWSET_ONLY) == (0, 1)
    header = (ROOT / "include" / "mi355rec_diag.h").read_text()
    assert "#define MI355REC_ROWSET_EXCLUDE 0u" in header and "#define MI355REC_ROWSET_ONLY 1u" in header
    for name in ("mi355rec_rowset_create", "mi355rec_sharded_rowset_create", "mi355rec_rowset_add", "mi355rec_rowset_count",
                 "mi355rec_rowset_destroy", "mi355rec_query_playlist_request_ext", "mi355rec_query_distance_request_ext",
                 "mi355rec_sharded_query_playlist_request_ext", "mi355rec_sharded_query_distance_request_ext"):
        assert name in capi.SIGNATURES and hasattr(engine_lib, name) and name + "(" in header, name


@pytest.fixture(scope="module")
def rowset_check(tmp_path_factory):
    """tests/rowset_check.cpp built with AddressSanitizer and UBSan (its own process: nothing is preloaded into python)."""
    exe = tmp_path_factory.mktemp("rowset") / "rowset_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           str(ROOT / "tests" / "rowset_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + p.stderr[-300:])
    return exe


def test_rowset_h_under_sanitizers(rowset_check):
    p = subprocess.run([str(rowset_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "rowset.h: ok" in p.stdout, p.stdout + p.stderr


def test_slice_against_numpy(rowset_check, tmp_path):
    """bit i of the slice [lo, hi) is bit lo + i of the source, the padding bits are 0, the count is the slice's popcount: lo and hi
    at every residue mod 32."""
    n_bits = 32 * 9 + 5
    rng = np.random.default_rng(3)
    words = rng.integers(0, 2 ** 32, size=(n_bits + 31) // 32, dtype=np.uint64).astype(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    pairs = []
    for lo_r in range(32):
        for hi_r in range(32):
            lo = 32 * int(rng.integers(0, 3)) + lo_r
            hi = 32 * int(rng.integers(4, 9)) + hi_r
            pairs.append((lo, hi))
    pairs += [(0, 0), (5, 5), (0, n_bits), (n_bits - 1, n_bits), (31, 33), (7, 8)]
    assert {lo % 32 for lo, _ in pairs} == set(range(32)) == {hi % 32 for _, hi in pairs}
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.asarray([n_bits, len(pairs)], np.int64).tobytes() + words.tobytes() + np.asarray(pairs, np.int64).tobytes())
    p = subprocess.run([str(rowset_check), "slice", str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = dst.read_bytes()
    at = 0
    for lo, hi in pairs:
        nw = (hi - lo + 31) // 32
        got = np.frombuffer(out, np.uint32, nw, at)
        at += 4 * nw
        count = int(np.frombuffer(out, np.int64, 1, at)[0])
        at += 8
        want = np.zeros(nw * 32, np.uint8)
        want[:hi - lo] = bits[lo:hi]
        assert np.array_equal(got, np.packbits(want, bitorder="little").view(np.uint32)), (lo, hi)
        assert count == int(bits[lo:hi].sum()), (lo, hi)
    assert at == len(out)
