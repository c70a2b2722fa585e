"""FEATURE FILTERS on a host without a GPU: the filtered playlist calls (K = 1 is the filtered single query) through the
node handle, served by the product's CPU backend (csrc/cpu_backend.cpp), the C-ABI's argument errors, the drop-in CLI's
--where and Recommender::recommendByIndexWhere through the shim.  Checked against the oracle (tests/filter_oracle.py):
identical ids, bit-equal scores.  Also what the built library says about playlist_scan_kernel, which carries the filter."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.filter_oracle import expected, expected_rows, pass_mask, raw_filter
from tests.labels_oracle import catalogue, check
from tests.playlist_oracle import expected_rows as playlist_rows


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")


@pytest.fixture(scope="module")
def node(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, _ = catalogue(20_000, 114, seed=11)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        yield nd, feats


WHERES = {
    "energy_high": {"energy": (0.5, 1.0)},                         # about half the rows
    "two_features": {1: (0.2, 0.9), "liveness": (0.0, 0.3)},       # about a fifth
    "narrow": {"tempo": (0.40, 0.41), 0: (0.0, 0.5)},              # about 0.5 %
}


@cpu_only
@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("wname", sorted(WHERES))
def test_filtered_playlists_match_the_oracle(node, k, wname):
    nd, feats = node
    where = WHERES[wname]
    rng = np.random.default_rng(k * 7 + len(wname))
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    excl = rng.integers(0, feats.shape[0], size=300)
    top = expected_rows(feats, rows, [], where, 200)[0]
    pick = top[::4][:50]
    excl[:pick.size] = pick              # (from the filtered top, where the exclusion matters)
    for topn in (1, 10, 1024):
        check(nd.query_playlist_topn(rows, topn, where=where), expected_rows(feats, rows, [], where, topn), f"{wname} k={k} top-{topn}")
        check(nd.query_playlist_topn(rows, topn, excl, where=where), expected_rows(feats, rows, excl, where, topn),
              f"{wname} k={k} top-{topn} excluded")
        check(nd.query_mean_topn(feats[rows], topn, excl, where=where), expected(feats, feats[rows], excl, where, topn),
              f"{wname} k={k} top-{topn} by value")
    got = nd.query_playlist_topn(rows, 50, where=where)[0]
    assert pass_mask(feats[got], where).all()


@cpu_only
def test_no_filter_is_the_unfiltered_call(node, engine_lib):
    from spotify_recommender_amd import capi
    nd, feats = node
    rows = np.array([3, 999, 15_000], np.int64)
    want = nd.query_playlist_topn(rows, 100, [5, 6])
    check(nd.query_playlist_topn(rows, 100, [5, 6], where={}), want, "active == 0")
    check(want, playlist_rows(feats, rows, [5, 6], 100), "oracle")
    # a NULL filter pointer, and active == 0 with bounds that would reject every row
    for flt in (None, ctypes.byref(raw_filter(capi, 0, np.full(12, 2.0), np.full(12, 3.0)))):
        idx = np.empty(100, np.int64)
        sc = np.empty(100, np.float32)
        c = ctypes.c_int(0)
        ex = np.array([5, 6], np.int64)
        assert engine_lib.mi355rec_sharded_query_playlist_topn_where(
            nd._h, rows.ctypes.data_as(ctypes.c_void_p), 3, ex.ctypes.data_as(ctypes.c_void_p), 2, flt, 100,
            idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c)) == 0
        check((idx[:c.value], sc[:c.value]), want, "NULL / inactive filter")
    # K = 1 with an all-pass filter is the single query
    got = nd.query_playlist_topn([99], 100, where={"energy": (-np.inf, np.inf)})
    single = nd.query_row_topn(99, 100)
    check(got, single, "one song, all-pass filter")


@cpu_only
def test_few_and_no_passing_rows(node, engine_lib):
    nd, feats = node
    few = {"danceability": (0.0, 0.02), "energy": (0.0, 0.05)}       # a handful of rows
    n_pass = int(pass_mask(feats, few).sum())
    assert 0 < n_pass < 100, n_pass
    idx, sc = nd.query_playlist_topn([7], 100, where=few)
    assert len(idx) == n_pass - (1 if pass_mask(feats[7:8], few)[0] else 0)
    check((idx, sc), expected_rows(feats, [7], [], few, 100), "few")
    # padding of the raw call: -1 / 0 past the count
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import make_filter
    flt = make_filter(few)
    out_i = np.full(100, 77, np.int64)
    out_s = np.full(100, 7.0, np.float32)
    c = ctypes.c_int(-5)
    rows = np.array([7], np.int64)
    assert engine_lib.mi355rec_sharded_query_playlist_topn_where(
        nd._h, rows.ctypes.data_as(ctypes.c_void_p), 1, None, 0, ctypes.byref(flt), 100, out_i.ctypes.data_as(ctypes.c_void_p),
        out_s.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c)) == capi.OK
    assert c.value == len(idx)
    assert (out_i[c.value:] == -1).all() and (out_s[c.value:] == 0).all()
    # nothing passes: count 0
    for none in ({"energy": (2.0, 3.0)}, {"mode": (0.25, 0.25)}):
        idx, sc = nd.query_mean_topn(feats[:2], 10, where=none)
        assert len(idx) == 0 and len(sc) == 0


@cpu_only
def test_special_values(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = oracle.mt19937_uniform(5, 1000)
    feats[20, 1] = np.nan                # NaN feature: fails any active bound on it
    feats[21, 1] = np.inf
    feats[22, 1] = -np.inf
    feats[23, 1] = -0.0
    feats[24, 1] = 0.0
    feats[25, 1] = 1e30
    feats[26:30] = 0.0                   # zero rows
    feats[40, 4] = np.nan                # NaN on another feature: fails only where that feature is constrained
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        cases = [
            {1: (-np.inf, np.inf)},       # every finite and infinite value passes, NaN fails
            {1: (0.0, np.inf)},
            {1: (-np.inf, 0.0)},
            {1: (-0.0, -0.0)},            # lo == hi; -0.0 equals +0.0
            {1: (0.0, 0.0), 4: (-1.0, 2.0)},
            {1: (np.inf, np.inf)},
            {4: (0.0, 1.0)},
            {1: (0.25, 0.25)},
        ]
        for i, where in enumerate(cases):
            for members in ([3], [3, 21, 40], [26]):
                check(nd.query_playlist_topn(members, 1024, where=where), expected_rows(feats, members, [], where, 1024),
                      f"case {i} members {members}")
            vecs = np.array([feats[3], feats[100]])
            check(nd.query_mean_topn(vecs, 50, where=where), expected(feats, vecs, [], where, 50), f"case {i} by value")
        idx = nd.query_playlist_topn([3], 1024, where={1: (-np.inf, np.inf)})[0]
        assert 20 not in idx and {21, 22, 23, 24, 25} <= set(idx.tolist())
        idx = nd.query_playlist_topn([3], 1024, where={1: (-0.0, -0.0)})[0]
        assert set(idx.tolist()) == {23, 24, 26, 27, 28, 29}


@cpu_only
def test_argument_errors(node, engine_lib):
    from spotify_recommender_amd import capi
    nd, feats = node
    L = engine_lib
    rows = np.array([1, 2], np.int64)
    idx = np.empty(10, np.int64)
    sc = np.empty(10, np.float32)
    c = ctypes.c_int(0)
    lo, hi = np.zeros(12), np.ones(12)
    nan_lo, nan_hi, swapped = lo.copy(), hi.copy(), lo.copy()
    nan_lo[3] = np.nan
    nan_hi[11] = np.nan
    swapped[5] = 1.5
    cases = [
        (raw_filter(capi, 1 << 12, lo, hi), "active mask"),
        (raw_filter(capi, 0x80000001, lo, hi), "active mask"),
        (raw_filter(capi, 1 << 3, nan_lo, hi), "NaN bound on feature 3"),
        (raw_filter(capi, 1 << 11, lo, nan_hi), "NaN bound on feature 11"),
        (raw_filter(capi, 1 << 5, swapped, hi), "feature 5 has lo"),
    ]
    for flt, msg in cases:
        for fn, members in ((L.mi355rec_sharded_query_playlist_topn_where, rows),
                            (L.mi355rec_sharded_query_mean_topn_where, feats[:2].copy())):
            rc = fn(nd._h, members.ctypes.data_as(ctypes.c_void_p), 2, None, 0, ctypes.byref(flt), 10,
                    idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c))
            assert rc == capi.ERR_INVALID_ARG, msg
            assert msg in L.mi355rec_sharded_last_error(nd._h).decode(), (msg, L.mi355rec_sharded_last_error(nd._h))
    # NaN or swapped bounds on a feature that is NOT active are not looked at
    ok = raw_filter(capi, 1 << 1, np.where(np.arange(12) == 1, 0.0, np.nan), np.where(np.arange(12) == 1, 1.0, -5.0))
    rc = L.mi355rec_sharded_query_playlist_topn_where(nd._h, rows.ctypes.data_as(ctypes.c_void_p), 2, None, 0, ctypes.byref(ok), 10,
                                                      idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                      ctypes.byref(c))
    assert rc == capi.OK
    # the playlist calls' own checks still come first / still apply
    good = ctypes.byref(raw_filter(capi, 1 << 1, lo, hi))
    for k, topn, n_ex, ex in ((0, 10, 0, None), (33, 10, 0, None), (2, 0, 0, None), (2, 1025, 0, None), (2, 10, 3, None),
                              (2, 10, -1, None)):
        r = np.arange(max(k, 1), dtype=np.int64)
        rc = L.mi355rec_sharded_query_playlist_topn_where(nd._h, r.ctypes.data_as(ctypes.c_void_p), k, ex, n_ex, good, topn,
                                                          idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                          ctypes.byref(c))
        assert rc == capi.ERR_INVALID_ARG, (k, topn, n_ex)
        assert L.mi355rec_sharded_last_error(nd._h)
    with pytest.raises(capi.Mi355Error):
        nd.query_playlist_topn([feats.shape[0]], 10, where={"energy": (0, 1)})
    with pytest.raises(capi.Mi355Error):
        nd.query_playlist_topn([1], 10, [-1], where={"energy": (0, 1)})
    # Python's own refusals: unknown names and indices
    with pytest.raises(ValueError):
        nd.query_playlist_topn([1], 10, where={"loudnes": (0, 1)})
    with pytest.raises(ValueError):
        nd.query_playlist_topn([1], 10, where={12: (0, 1)})
    # a good call after the errors still answers
    check(nd.query_playlist_topn([1, 2], 10, where={"energy": (0.3, 0.6)}),
          expected_rows(feats, [1, 2], [], {"energy": (0.3, 0.6)}, 10), "after errors")


def test_kernel_budget_in_the_built_library(engine_lib):
    """The filter lives in playlist_scan_kernel: the library keeps its 60 kernels, none with scratch, and the kernel keeps
    two 512-thread workgroups per CU (<= 128 VGPRs, <= 80 KB of LDS)."""
    from spotify_recommender_amd import build
    kernels = build.kernel_metadata(build.LIB_ENGINE)
    assert len(kernels) == 60, len(kernels)
    assert all(k["scratch"] == 0 for k in kernels)
    pl = [k for k in kernels if "playlist_scan_kernel" in k["name"]]
    assert len(pl) == 1, pl
    assert pl[0]["vgpr"] <= 128 and pl[0]["lds"] <= 80 * 1024, pl


# ---- the drop-in: CLI and Recommender through the shim --------------------------------------------------------------
COLS = ("danceability", "energy", "key", "loudness", "mode", "speechiness", "acousticness", "instrumentalness", "liveness",
        "valence", "tempo")


def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _shim():
    from spotify_recommender_amd import build
    build.build_shim()
    shim = ctypes.CDLL(str(build.LIB_SHIM))
    shim.shim_load.restype = ctypes.c_void_p
    shim.shim_load.argtypes = [ctypes.c_char_p]
    shim.shim_free.argtypes = [ctypes.c_void_p]
    shim.shim_initialize.argtypes = [ctypes.c_void_p]
    shim.shim_song_count.restype = ctypes.c_int64
    shim.shim_song_count.argtypes = [ctypes.c_void_p]
    shim.shim_song_features.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    shim.shim_recommend_by_index_where.restype = ctypes.c_int64
    shim.shim_recommend_by_index_where.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    shim.shim_recommend_for_playlist_where.restype = ctypes.c_int64
    shim.shim_recommend_for_playlist_where.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    return shim


def _served_matrix(shim, path):
    h = shim.shim_load(str(path).encode())
    assert h
    try:
        n = shim.shim_song_count(h)
        feats = np.zeros((n, 12), np.float32)
        g = ctypes.c_int(0)
        for i in range(n):
            shim.shim_song_features(h, i, feats[i].ctypes.data, ctypes.byref(g))
    finally:
        shim.shim_free(h)
    return feats


def _ids(stdout):
    return [l.split("ID:", 1)[1].strip() for l in stdout.split("Recommendations:", 1)[1].splitlines() if l.strip().startswith("ID:")]


def test_cli_where_on_the_sample_csv(engine_lib, golden_dir, tmp_path):
    shim = _shim()
    shutil.copy(golden_dir / "sample_songs.csv", tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    feats = _served_matrix(shim, tmp_path / "songs_data.bin")
    track_ids = [l.split(",", 1)[0] for l in (tmp_path / "songs.csv").read_text().splitlines()[1:]]
    where = {"energy": (0.0, 0.6), "liveness": (0.0, 0.8)}
    args = ["--where", "energy=0:0.6", "--where", "liveness=0:0.8"]
    p = _run(["--id", track_ids[0], "-n", "10", *args], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    want = expected_rows(feats, [0], [], where, 10)[0]
    assert want.size > 0
    assert _ids(p.stdout) == [track_ids[i] for i in want], p.stdout
    # by name, and a playlist
    name = (tmp_path / "songs.csv").read_text().splitlines()[2].split(",")[1]
    p = _run(["--song", name, *args], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    want = expected_rows(feats, [1], [], where, 10)[0]
    assert want.size > 0
    assert _ids(p.stdout) == [track_ids[i] for i in want], p.stdout
    p = _run(["--playlist", f"{track_ids[0]},{track_ids[3]}", "--where", "danceability=0:0.5", "-n", "3"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    want = expected_rows(feats, [0, 3], [], {"danceability": (0.0, 0.5)}, 3)[0]
    assert want.size > 0
    assert _ids(p.stdout) == [track_ids[i] for i in want], p.stdout
    # refusals: with --genre, unknown names, malformed ranges, lo > hi
    for bad, msg in ((["--genre", "dance", "--where", "energy=0:1"], "--genre"),
                     (["--where", "genre=0:1"], "unknown feature"),
                     (["--where", "energy=0.5"], "NAME=LO:HI"),
                     (["--where", "energy=a:1"], "numbers"),
                     (["--where", "energy=0.9:0.1"], "")):
        p = _run(["--id", track_ids[0], *bad], tmp_path)
        assert p.returncode == 1, (bad, p.stdout)
        assert msg in p.stderr, (bad, p.stderr)
    # nothing passes: no recommendations, exit 1
    p = _run(["--id", track_ids[0], "--where", "energy=2:3"], tmp_path)
    assert p.returncode == 1
    # the usage text names the filter and its units
    p = _run([], tmp_path)
    assert "--where NAME=LO:HI" in p.stdout and "normalised" in p.stdout


def test_recommender_where_through_the_shim(engine_lib, golden_dir, tmp_path):
    shim = _shim()
    shutil.copy(golden_dir / "sample_songs.csv", tmp_path / "songs.csv")
    assert _run(["--preprocess", "songs.csv"], tmp_path).returncode == 0
    feats = _served_matrix(shim, tmp_path / "songs_data.bin")
    h = shim.shim_load(str(tmp_path / "songs_data.bin").encode())
    assert h
    try:
        assert shim.shim_initialize(h) == 1

        def by_index(idx, topn, ranges):
            f = np.array([r[0] for r in ranges], np.int32)
            lo = np.array([r[1] for r in ranges], np.float32)
            hi = np.array([r[2] for r in ranges], np.float32)
            out = np.full(16, -7, np.int32)
            scores = np.zeros(16, np.float32)
            n = shim.shim_recommend_by_index_where(h, idx, topn, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(ranges),
                                                   out.ctypes.data, scores.ctypes.data, 16)
            return out[:n].astype(np.int64), scores[:n]

        # two ranges on one feature intersect
        check(by_index(2, 10, [(1, 0.0, 0.9), (1, 0.4, 1.0)]), expected_rows(feats, [2], [], {1: (0.4, 0.9)}, 10), "intersect")
        check(by_index(2, 10, []), expected_rows(feats, [2], [], {}, 10), "no ranges")
        for bad in ([(12, 0, 1)], [(-1, 0, 1)], [(1, 0.6, 0.5)], [(1, np.nan, 1.0)], [(1, 0.0, 0.2), (1, 0.5, 1.0)]):
            assert len(by_index(2, 10, bad)[0]) == 0, bad
        songs = np.array([0, 3], np.int32)
        f = np.array([0], np.int32)
        lo = np.array([0.0], np.float32)
        hi = np.array([0.5], np.float32)
        excl = np.array([1], np.int32)
        out = np.zeros(16, np.int32)
        scores = np.zeros(16, np.float32)
        n = shim.shim_recommend_for_playlist_where(h, songs.ctypes.data, 2, 10, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, 1,
                                                   excl.ctypes.data, 1, out.ctypes.data, scores.ctypes.data, 16)
        check((out[:n].astype(np.int64), scores[:n]), expected_rows(feats, [0, 3], [1], {0: (0.0, 0.5)}, 10), "playlist")
        assert n > 0
    finally:
        shim.shim_free(h)
