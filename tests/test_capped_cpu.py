"""GROUP CAPS on a host without a GPU: "at most M per group" through the node handle (served by the product's CPU backend,
csrc/cpu_backend.cpp), the C-ABI's argument errors, the C++ drop-in through its shim and the CLI's --max-per-artist.
Checked against the oracle (tests/capped_oracle.py): identical ids, bit-equal relevance, bit-equal mmr, the count and P'."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests.capped_oracle import (WHERE, cap_holds, check3, check4, default_pool, in_order_capped, layouts, pools, rerank_capped, run_variant,
                                 variant_pool, variants)
from tests.diverse_oracle import rerank
from tests.labels_oracle import check


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

LAMBDAS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def node(engine_lib, golden_dir):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = np.ascontiguousarray(np.load(golden_dir / "catalogue4096.npz")["feats"])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        yield nd, feats, layouts(feats.shape[0])


def test_the_two_forms_of_the_oracle_agree(node):
    """lambda = 1: the greedy loop with the eligibility rule is the closed form (rank in group below the cap, first topn)."""
    nd, feats, lay = node
    rng = np.random.default_rng(1)
    for v in variants(rng, feats, 3):
        pidx, prel = variant_pool(feats, v, 1024)
        for name, g in lay.items():
            for topn, pool, m in ((1, 1, 1), (10, 40, 1), (10, 40, 2), (10, 1024, 3), (256, 1024, 2), (256, 256, 256), (300, 1024, 1)):
                a = rerank_capped(feats, pidx[:pool], prel[:pool], g, 1.0, m, topn)
                b = in_order_capped(pidx[:pool], prel[:pool], g, m, topn)
                check3(a, b, f"{v[0]} {name} top-{topn} pool {pool} M {m}")
                assert cap_holds(a[0], g, m)


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("topn", [1, 10, 256])
def test_capped_queries_match_the_oracle(node, k, topn):
    nd, feats, lay = node
    rng = np.random.default_rng(k * 1000 + topn)
    vs = list(variants(rng, feats, k))
    vs = [vs[0], vs[3], vs[2]]                                   # by row; by value, signed weights, excluded, filtered; dislikes
    full = [variant_pool(feats, v, 1024) for v in vs]            # (a smaller pool is a prefix: canonical order)
    short = 0
    try:
        for name, g in lay.items():
            nd.set_groups(g)
            for v, (pidx, prel) in zip(vs, full):
                for pool in pools(topn):
                    for lam in LAMBDAS:
                        for m in sorted({1, 2, topn}):
                            got = run_variant(nd, v, lam, pool, m, topn)
                            want = rerank_capped(feats, pidx[:pool], prel[:pool], g, lam, m, topn)
                            what = f"k={k} top-{topn} pool {pool} lambda {lam} M {m} {name} {v[0]}"
                            check4(got, want, min(pool, pidx.size), what)
                            assert cap_holds(got[0], g, m), what
                            short += got[0].size < min(topn, pool, pidx.size)
    finally:
        nd.set_groups(None)
    assert topn == 1 or short > 0, "the grid must hold cases in which the cap leaves fewer than topn"


def test_identities(node):
    nd, feats, lay = node
    rows, w, excl = [5, 777, 3000], [1.0, -0.5, 2.0], [3, 4, 5]
    kw = dict(exclude=excl, where=WHERE, weights=w, return_mmr=True)
    try:
        for topn, pool in ((1, 8), (10, 40), (10, 1024), (256, 1024)):
            for lam in (0.0, 0.3, 0.7, 1.0):
                plain = nd.query_playlist_topn_diverse(rows, topn, lam, pool, **kw)
                # no cap is the diverse call: max_per_group >= topn, or every group -1
                for name in ("row % 7", "row // 3", "a third -1", "near 2^31"):
                    nd.set_groups(lay[name])
                    for m in (topn, topn + 1, 2 ** 31 - 1):
                        check3(nd.query_playlist_topn_capped(rows, topn, m, lam, pool, **kw), plain, f"M {m} >= top-{topn} {name}")
                nd.set_groups(lay["all -1"])
                for m in (1, 2):
                    check3(nd.query_playlist_topn_capped(rows, topn, m, lam, pool, **kw), plain, f"all -1, M {m}, top-{topn}")
            # lambda = 1 is the in-order walk, out_mmr == out_score
            pool_ids, pool_rel = nd.query_playlist_topn(rows, pool, excl, where=WHERE, weights=w)
            for name, g in lay.items():
                nd.set_groups(g)
                for m in (1, 2, 3):
                    got = nd.query_playlist_topn_capped(rows, topn, m, 1.0, pool, **kw)
                    check3(got, in_order_capped(pool_ids, pool_rel, g, m, topn), f"lambda 1 {name} M {m} top-{topn} pool {pool}")
                    assert np.array_equal(got[1].view(np.uint32), got[2].view(np.uint32))
                    # the cap always holds
                    for lam in (0.0, 0.5):
                        ids = nd.query_playlist_topn_capped(rows, topn, m, lam, pool, exclude=excl, where=WHERE, weights=w)[0]
                        assert cap_holds(ids, g, m), (name, m, lam)
    finally:
        nd.set_groups(None)


def test_defaults_and_return_shapes(node):
    nd, feats, lay = node
    g = lay["row // 3"]
    nd.set_groups(g)
    try:
        from tests.weighted_oracle import expected_rows as pool_rows
        for topn in (1, 10, 200):
            got = nd.query_playlist_topn_capped([4, 9], topn, 1)             # lam = 1.0, pool = min(1024, 8 topn)
            assert len(got) == 2
            pidx, prel = pool_rows(feats, [4, 9], [1.0, 1.0], [], default_pool(topn))
            check(got, in_order_capped(pidx, prel, g, 1, topn)[:2], f"defaults, top-{topn}")
        assert default_pool(10) == 80 and default_pool(200) == 1024 and default_pool(1) == 8
        assert len(nd.query_mean_topn_capped(feats[[4, 9]], 5, 1, return_mmr=True)) == 3
        assert len(nd.query_mean_topn_capped(feats[[4, 9]], 5, 1, return_pool_rows=True)) == 3
        assert len(nd.query_mean_topn_capped(feats[[4, 9]], 5, 1, return_mmr=True, return_pool_rows=True)) == 4
    finally:
        nd.set_groups(None)


def test_out_pool_rows_tells_the_two_ways_of_running_out(node, engine_lib):
    nd, feats, lay = node
    nd.set_groups(lay["row % 7"])
    try:
        # seven groups, one each: the pool ran out (P' == pool): raise pool ... which does not help here either
        for pool in (40, 1024):
            ids, rel, p = nd.query_playlist_topn_capped([7, 8], 10, 1, 0.5, pool, return_pool_rows=True)
            assert ids.size == 7 and p == pool
        # a tight filter: the catalogue has no more (P' < pool)
        tight = {0: (0.0, 0.05), 1: (0.0, 0.3)}
        admissible = int(np.count_nonzero((feats[:, 0] >= 0) & (feats[:, 0] <= 0.05) & (feats[:, 1] >= 0) & (feats[:, 1] <= 0.3)))
        assert 7 < admissible < 200
        nd.set_groups(lay["row // 3"])
        for lam in (0.5, 1.0):
            ids, rel, mmr, p = nd.query_playlist_topn_capped([7, 8], 256, 2, lam, 1024, where=tight, return_mmr=True, return_pool_rows=True)
            assert admissible - 2 <= p <= admissible and ids.size <= p < 1024
            from tests.weighted_oracle import expected_rows as pool_rows
            pidx, prel = pool_rows(feats, [7, 8], [1.0, 1.0], [], 1024, tight)
            check3((ids, rel, mmr), rerank_capped(feats, pidx, prel, lay["row // 3"], lam, 2, 256), f"tight filter, lambda {lam}")
        # the raw call: count, padding -1 / 0 / 0, NULL out pointers
        from spotify_recommender_amd.engine import make_filter
        flt = make_filter(tight)
        rows = np.array([7, 8], np.int64)
        idx, sc, mm = np.full(256, 7, np.int64), np.full(256, 7, np.float32), np.full(256, 7, np.float32)
        c, p = ctypes.c_int(-1), ctypes.c_int(-1)
        fn = engine_lib.mi355rec_sharded_query_playlist_topn_capped
        rc = fn(nd._h, rows.ctypes.data_as(ctypes.c_void_p), None, 2, None, 0, ctypes.byref(flt), ctypes.c_float(0.5), 1024, 2, 256,
                idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), mm.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c),
                ctypes.byref(p))
        assert rc == 0 and 0 < c.value <= p.value < 256
        assert np.all(idx[:c.value] >= 0) and np.all(idx[c.value:] == -1)
        assert not sc[c.value:].view(np.uint32).any() and not mm[c.value:].view(np.uint32).any()
        rc = fn(nd._h, rows.ctypes.data_as(ctypes.c_void_p), None, 2, None, 0, None, ctypes.c_float(1.0), 40, 1, 10,
                idx.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(c), None)
        assert rc == 0 and c.value == 10
    finally:
        nd.set_groups(None)


def test_argument_errors(node, engine_lib):
    from spotify_recommender_amd import capi
    nd, feats, lay = node
    n = feats.shape[0]
    ones2 = np.ones((2, 12), np.float32)

    def refused(call, word=None):
        with pytest.raises(capi.Mi355Error) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value)
        if word:
            assert word in str(e.value), str(e.value)

    # a handle without groups
    refused(lambda: nd.query_playlist_topn_capped([1, 2], 10, 2), "groups")
    refused(lambda: nd.query_mean_topn_capped(ones2, 10, 2), "groups")
    # set_groups: the wrong length, a value below -1; a failure leaves the previous groups in place
    g = lay["row // 3"]
    nd.set_groups(g)
    try:
        want = nd.query_playlist_topn_capped([1, 2], 10, 1, 0.5, 40, return_mmr=True)
        refused(lambda: nd.set_groups(g[:-1]))
        bad = g.copy()
        bad[17] = -2
        refused(lambda: nd.set_groups(bad))
        with pytest.raises(ValueError):
            nd.set_groups(np.array([2 ** 31] * n, np.int64))
        with pytest.raises(ValueError):
            nd.set_groups(np.zeros(n, np.float32))
        check3(nd.query_playlist_topn_capped([1, 2], 10, 1, 0.5, 40, return_mmr=True), want, "the previous groups stay")
        bad_calls = [
            lambda: nd.query_playlist_topn_capped([1, 2], 10, 0),
            lambda: nd.query_playlist_topn_capped([1, 2], 10, -1),
            lambda: nd.query_mean_topn_capped(ones2, 10, 0),
            # inherited from the diversified calls
            lambda: nd.query_playlist_topn_capped([1, 2], 10, 2, np.nan, 40),
            lambda: nd.query_playlist_topn_capped([1, 2], 10, 2, -0.1, 40),
            lambda: nd.query_mean_topn_capped(ones2, 10, 2, 1.5, 40),
            lambda: nd.query_playlist_topn_capped([1, 2], 10, 2, 0.5, 9),
            lambda: nd.query_mean_topn_capped(ones2, 10, 2, 0.5, 1025),
            lambda: nd.query_playlist_topn_capped([1, 2], 0, 2, 0.5, 40),
            lambda: nd.query_playlist_topn_capped([1, 2], 10, 2, 0.5, 40, weights=[0.0, 0.0]),
            lambda: nd.query_playlist_topn_capped([1], 10, 2, 0.5, 40, where={1: (0.9, 0.1)}),
            lambda: nd.query_playlist_topn_capped(list(range(33)), 10, 2, 0.5, 40),
            lambda: nd.query_playlist_topn_capped([n], 10, 2, 0.5, 40),
            lambda: nd.query_playlist_topn_capped([1], 10, 2, 0.5, 40, exclude=[n]),
        ]
        for call in bad_calls:
            refused(call)
        for bad_m in ("2", 2.0, None, True):
            with pytest.raises(ValueError):
                nd.query_playlist_topn_capped([1, 2], 10, bad_m)
        # raw calls: a message that names what was wrong
        rows = np.array([1, 2], np.int64)
        idx = np.empty(16, np.int64)
        c = ctypes.c_int(0)
        for fn, members in (("mi355rec_sharded_query_playlist_topn_capped", rows), ("mi355rec_sharded_query_mean_topn_capped", ones2)):
            rc = getattr(engine_lib, fn)(nd._h, members.ctypes.data_as(ctypes.c_void_p), None, 2, None, 0, None, ctypes.c_float(0.5), 40, 0, 10,
                                         idx.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(c), None)
            assert rc == capi.ERR_INVALID_ARG and b"max_per_group" in engine_lib.mi355rec_sharded_last_error(nd._h)
        # a good call after the errors still answers; a second set_groups replaces the groups; None drops them
        check3(nd.query_playlist_topn_capped([1, 2], 10, 1, 0.5, 40, return_mmr=True), want, "after the errors")
        nd.set_groups(lay["row % 7"])
        other = nd.query_playlist_topn_capped([1, 2], 10, 1, 0.5, 40, return_mmr=True)
        assert other[0].size == 7 and other[0].tolist() != want[0].tolist()
    finally:
        nd.set_groups(None)
    refused(lambda: nd.query_playlist_topn_capped([1, 2], 10, 2), "groups")
    # the uncapped calls never needed groups
    check3(nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, return_mmr=True),
           rerank(feats, *variant_pool(feats, ("", np.array([1, 2]), None, None, None, None), 40), 0.5, 10), "diverse without groups")


# ---- the C++ drop-in (through its shim) and the CLI ---------------------------------------------------------------------
def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _shim():
    from tests.test_diverse_cpu import _shim as diverse_shim
    shim = diverse_shim()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    shim.shim_recommend_capped.restype = ctypes.c_int64
    shim.shim_recommend_capped.argtypes = [P, I, I, I, F, I, P, P, P, I, P, P, P, ctypes.c_int64]
    shim.shim_recommend_for_playlist_capped.restype = ctypes.c_int64
    shim.shim_recommend_for_playlist_capped.argtypes = [P, P, I, P, I, I, P, P, P, I, P, I, F, I, I, P, P, ctypes.c_int64]
    shim.shim_artist_groups.argtypes = [P, P]
    shim.shim_song_string.restype = ctypes.c_int64
    shim.shim_song_string.argtypes = [P, ctypes.c_int64, I, ctypes.c_char_p, ctypes.c_int64]
    return shim


def _write_csv(path, rows=600, seed=4):
    """The sample CSV of the playlist tests with artists that exercise the key: 'Artist a' alone, or with guests after ';'."""
    from tests.test_playlist_cpu import GENRES
    rng = np.random.default_rng(seed)
    lines = ["track_id,track_name,artists,danceability,energy,key,loudness,mode,speechiness,acousticness,"
             "instrumentalness,liveness,valence,tempo,track_genre"]
    for i in range(rows):
        r = rng.random(10)
        artists = f"Artist {i % 23}" + (f";Guest {i % 5}" if i % 4 == 0 else "") + (";Artist 1" if i % 9 == 0 else "")
        lines.append(f"t{i:04d},Song {i:04d},{artists},{r[0]:.3f},{r[1]:.3f},{int(r[2] * 11)},{-60 * r[3]:.3f},"
                     f"{int(r[4] * 2)},{r[5]:.4f},{r[6]:.5f},{r[7] ** 6:.6f},{r[8]:.4f},{r[9]:.4f},{60 + 140 * r[2]:.3f},"
                     f"{GENRES[(i // 40) % len(GENRES)]}")
    path.write_text("\n".join(lines) + "\n")


@pytest.fixture()
def sample(engine_lib, tmp_path):
    from tests.test_weighted_cpu import _served_matrix
    shim = _shim()
    _write_csv(tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    feats = _served_matrix(shim, tmp_path / "songs_data.bin")
    track_ids = [l.split(",", 1)[0] for l in (tmp_path / "songs.csv").read_text().splitlines()[1:]]
    # the primary artist of every song as the file holds it, and the groups they make (ids by first appearance)
    h = shim.shim_load(str(tmp_path / "songs_data.bin").encode())
    try:
        buf = ctypes.create_string_buffer(256)
        primary = []
        for i in range(feats.shape[0]):
            n = shim.shim_song_string(h, i, 2, buf, 256)
            primary.append(buf.raw[:n].decode().split(";", 1)[0])
    finally:
        shim.shim_free(h)
    first = {}
    groups = np.array([first.setdefault(a, len(first)) if a else -1 for a in primary], np.int32)
    return shim, feats, track_ids, tmp_path, primary, groups


def _ids(stdout):
    return [l.split("ID:", 1)[1].strip() for l in stdout.split("Recommendations:", 1)[1].splitlines() if l.strip().startswith("ID:")]


def _expected(feats, groups, rows, weights, exclude, where, lam, pool, m, topn):
    from tests.weighted_oracle import expected_rows as pool_rows
    w = np.ones(len(rows), np.float32) if weights is None else weights
    pidx, prel = pool_rows(feats, rows, w, exclude, pool, where)
    return rerank_capped(feats, pidx, prel, groups, lam, m, topn)


def test_recommender_capped_through_the_shim(sample):
    shim, feats, t, cwd, primary, groups = sample
    assert len(set(primary)) == 23 and all(primary)
    h = shim.shim_load(str(cwd / "songs_data.bin").encode())
    assert h
    try:
        assert shim.shim_initialize(h) == 1
        derived = np.full(feats.shape[0], -9, np.int32)
        shim.shim_artist_groups(h, derived.ctypes.data)
        assert derived.tolist() == groups.tolist()                              # the bytes before the first ';', ids by first appearance

        def arrays(ranges, exclude):
            f = np.array([r[0] for r in ranges] or [0], np.int32)
            lo = np.array([r[1] for r in ranges] or [0], np.float32)
            hi = np.array([r[2] for r in ranges] or [0], np.float32)
            return f, lo, hi, np.array(list(exclude) or [0], np.int32)

        def capped(song, topn, m, lam=1.0, pool=0, ranges=(), group_ids=None):
            f, lo, hi, _ = arrays(ranges, ())
            out, sc = np.full(64, -7, np.int32), np.zeros(64, np.float32)
            n = shim.shim_recommend_capped(h, song, topn, m, lam, pool, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(ranges),
                                           group_ids.ctypes.data if group_ids is not None else None, out.ctypes.data, sc.ctypes.data, 64)
            return out[:max(n, 0)].astype(np.int64), sc[:max(n, 0)]

        def playlist(songs, weights, topn, m, lam=1.0, pool=0, ranges=(), exclude=()):
            s, w = np.array(songs, np.int32), np.array(list(weights) or [0], np.float32)
            f, lo, hi, ex = arrays(ranges, exclude)
            out, sc = np.full(64, -7, np.int32), np.zeros(64, np.float32)
            n = shim.shim_recommend_for_playlist_capped(h, s.ctypes.data, len(songs), w.ctypes.data, len(weights), topn, f.ctypes.data,
                                                        lo.ctypes.data, hi.ctypes.data, len(ranges), ex.ctypes.data, len(exclude), lam, pool,
                                                        m, out.ctypes.data, sc.ctypes.data, 64)
            return out[:max(n, 0)].astype(np.int64), sc[:max(n, 0)]

        def per_artist(ids):
            names = [primary[i] for i in ids.tolist()]
            return max(names.count(a) for a in set(names))

        for m in (1, 2, 3):
            got = capped(4, 10, m)                                              # lambda 1, the default pool 8 x N
            check(got, _expected(feats, groups, [4], None, [], None, 1.0, 80, m, 10)[:2], f"recommendByIndexCapped M {m}")
            assert got[0].size == 10 and per_artist(got[0]) <= m
            got = capped(4, 20, m, 0.5, 120, [(1, 0.0, 0.9)])
            check(got, _expected(feats, groups, [4], None, [], {1: (0.0, 0.9)}, 0.5, 120, m, 20)[:2], f"lambda 0.5, filtered, M {m}")
            assert per_artist(got[0]) <= m
        assert per_artist(capped(4, 10, 10)[0]) > 1                            # the sample does repeat artists without the cap
        w = [1.0, -0.75, 0.25]
        got = playlist([0, 3, 5], w, 12, 2, 0.7, 60, [(1, 0.0, 0.8)], [1, 2])
        check(got, _expected(feats, groups, [0, 3, 5], w, [1, 2], {1: (0.0, 0.8)}, 0.7, 60, 2, 12)[:2], "playlist, weighted, filtered")
        assert per_artist(got[0]) <= 2
        check(playlist([0, 3], [], 10, 1), _expected(feats, groups, [0, 3], None, [], None, 1.0, 80, 1, 10)[:2], "playlist, defaults")
        # the pool runs out: 23 artists, one each
        assert capped(4, 30, 1, 1.0, 1024 if feats.shape[0] > 1024 else feats.shape[0] - 1)[0].size == 23
        # setGroupIds: other groups, another answer
        other = (np.arange(feats.shape[0]) % 3).astype(np.int32)
        got = capped(4, 10, 2, 1.0, 0, (), other)
        check(got, _expected(feats, other, [4], None, [], None, 1.0, 80, 2, 10)[:2], "setGroupIds")
        assert got[0].size == 6
        # bad input: {} (and a message on stderr)
        assert capped(4, 10, 0)[0].size == 0
        assert capped(4, 10, -3)[0].size == 0
        assert capped(4, 10, 2, float("nan"))[0].size == 0
        assert capped(4, 10, 2, 0.5, 9)[0].size == 0
        assert capped(-1, 10, 2)[0].size == 0
        assert playlist([0, 3], [1.0], 10, 2)[0].size == 0
        bad = other.copy()
        bad[3] = -2
        f, lo, hi, _ = arrays((), ())
        out = np.zeros(64, np.int32)
        assert shim.shim_recommend_capped(h, 4, 10, 2, 1.0, 0, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, 0, bad.ctypes.data,
                                          out.ctypes.data, None, 64) == -1
        check(capped(4, 10, 2), _expected(feats, other, [4], None, [], None, 1.0, 80, 2, 10)[:2], "after the refusals")
    finally:
        shim.shim_free(h)


def test_cli_max_per_artist(sample):
    shim, feats, t, cwd, primary, groups = sample
    artist = dict(zip(t, primary))
    p = _run(["--id", t[4], "--max-per-artist", "1", "-n", "8"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    ids = _ids(p.stdout)
    assert ids == [t[i] for i in _expected(feats, groups, [4], None, [], None, 1.0, 64, 1, 8)[0]], p.stdout
    assert len({artist[i] for i in ids}) == 8
    assert "per artist" in p.stdout
    # the plain result repeats an artist here, so the cap did something
    plain = _ids(_run(["--id", t[4], "-n", "8"], cwd).stdout)
    assert len({artist[i] for i in plain}) < 8 and ids != plain
    # --song finds the same song
    assert _ids(_run(["--song", "Song 0004", "--max-per-artist", "1", "-n", "8"], cwd).stdout) == ids
    # with --where, --diverse and --pool
    where = {"energy": (0.0, 0.9)}
    p = _run(["--id", t[4], "--where", "energy=0:0.9", "--diverse", "0.5", "--pool", "100", "--max-per-artist", "2", "-n", "12"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in _expected(feats, groups, [4], None, [], where, 0.5, 100, 2, 12)[0]], p.stdout
    # --playlist with --dislike and --weights
    liked, disliked = [0, 3, 6], [9, 12]
    lk, dl = ",".join(t[i] for i in liked), ",".join(t[i] for i in disliked)
    p = _run(["--playlist", lk, "--dislike", dl, "--weights", "2,0.5,1", "--max-per-artist", "1", "--diverse", "0.7", "-n", "6"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    want = _expected(feats, groups, liked + disliked, np.array([2, 0.5, 1, -0.5, -0.5], np.float32), [], None, 0.7, 48, 1, 6)[0]
    assert _ids(p.stdout) == [t[i] for i in want], p.stdout
    p = _run(["--playlist", lk, "--max-per-artist", "2", "-n", "6"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in _expected(feats, groups, liked, None, [], None, 1.0, 48, 2, 6)[0]], p.stdout
    # the pool runs out: fewer than asked, still a success
    p = _run(["--id", t[4], "--max-per-artist", "1", "-n", "40"], cwd)
    assert p.returncode == 0 and len(_ids(p.stdout)) == 23
    # the refusals: exit status 1 and a message
    for bad, msg in ((["--max-per-artist", "0"], "--max-per-artist"), (["--max-per-artist", "-2"], "--max-per-artist"),
                     (["--max-per-artist", "x"], "--max-per-artist"), (["--max-per-artist", "1.5"], "--max-per-artist"),
                     (["--max-per-artist"], "needs a value"), (["--max-per-artist", "2", "--genre", "pop"], "--genre"),
                     (["--max-per-artist", "2", "--pool", "4", "-n", "5"], "--pool")):
        p = _run(["--id", t[4], *bad], cwd)
        assert p.returncode == 1, (bad, p.stdout)
        assert msg in p.stderr, (bad, p.stderr)
    p = _run(["--playlist", lk, "--max-per-artist", "0"], cwd)
    assert p.returncode == 1 and "--max-per-artist" in p.stderr
    assert "--max-per-artist" in _run([], cwd).stdout
