"""DIVERSIFIED TOP-N on a host without a GPU: MMR re-ranking through the node handle (served by the product's CPU backend,
csrc/cpu_backend.cpp), the C-ABI's argument errors, the C++ drop-in through its shim and the CLI's --diverse / --pool.
Checked against the oracle (tests/diverse_oracle.py): identical ids, bit-equal relevance, bit-equal mmr."""
import ctypes
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.diverse_oracle import (LAMBDAS, WHERE, check3, default_pool, expected, expected_rows, mean_pairwise, pools, rerank, run_variant,
                                   variant_pool, variants)
from tests.labels_oracle import catalogue, check
from tests.weighted_oracle import expected as pool_expected


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")



@pytest.fixture(scope="module")
def node(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, _ = catalogue(20_000, 114, seed=13)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        yield nd, feats


@pytest.mark.parametrize("k", [1, 2, 7, 32])
@pytest.mark.parametrize("topn", [1, 10, 256])
def test_diverse_queries_match_the_oracle(node, k, topn):
    nd, feats = node
    rng = np.random.default_rng(k * 1000 + topn)
    for v in variants(rng, feats, k):
        for pool in pools(topn):
            pidx, prel = variant_pool(feats, v, pool)
            for lam in LAMBDAS:
                check3(run_variant(nd, feats, v, lam, pool, topn), rerank(feats, pidx, prel, lam, topn),
                       f"k={k} top-{topn} pool {pool} lambda {lam} {v[0]}")


def test_the_oracle_entry_points_agree_with_the_grid_helpers(node):
    """tests/diverse_oracle.expected / expected_rows (what the other suites call) against one library call each."""
    nd, feats = node
    rows, w, excl = [5, 777, 12_345], [1.0, -0.5, 2.0], [3, 4, 5]
    check3(nd.query_playlist_topn_diverse(rows, 10, 0.5, 40, exclude=excl, where=WHERE, weights=w, return_mmr=True),
           expected_rows(feats, rows, w, excl, WHERE, 0.5, 40, 10), "by row")
    check3(nd.query_mean_topn_diverse(feats[rows], 10, 0.5, 40, return_mmr=True), expected(feats, feats[rows], None, [], None, 0.5, 40, 10),
           "by value")
    # pool=None is min(1024, max(topn, 4 * topn)); without return_mmr two arrays come back
    for topn in (1, 10, 300):
        got = nd.query_playlist_topn_diverse(rows, topn, 0.7)
        assert len(got) == 2
        check(got, expected_rows(feats, rows, None, [], None, 0.7, default_pool(topn), topn)[:2], f"default pool, top-{topn}")
    assert default_pool(300) == 1024 and default_pool(10) == 40


@pytest.mark.parametrize("k", [1, 7])
def test_identities_lambda_one_and_pool_equal_topn(node, k):
    nd, feats = node
    rng = np.random.default_rng(90 + k)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    w = rng.normal(0.0, 1.0, k).astype(np.float32)
    excl = rng.integers(0, feats.shape[0], size=50)
    for topn in (1, 10, 256):
        plain = nd.query_playlist_topn(rows, topn, excl, where=WHERE, weights=w)
        for pool in pools(topn):
            idx, rel, mmr = nd.query_playlist_topn_diverse(rows, topn, 1.0, pool, exclude=excl, where=WHERE, weights=w, return_mmr=True)
            check((idx, rel), plain, f"lambda 1, top-{topn} pool {pool}")
            assert np.array_equal(mmr.view(np.uint32), rel.view(np.uint32))
        for lam in (0.0, 0.3, 0.7):
            idx, rel = nd.query_playlist_topn_diverse(rows, topn, lam, topn, exclude=excl, where=WHERE, weights=w)
            order = np.argsort(idx)
            want = np.argsort(plain[0])
            assert idx[order].tolist() == plain[0][want].tolist(), f"pool == topn is a permutation (lambda {lam}, top-{topn})"
            assert np.array_equal(rel[order].view(np.uint32), plain[1][want].view(np.uint32))
            assert idx[0] == plain[0][0]                                        # the first pick is pool row 0


def test_duplicates_and_ties_go_by_pool_position(node):
    nd, feats = node
    # rows 100..109 copy row 99.  Query a row that is none of them, with the copies inside the pool: once one copy is picked
    # the others carry pen = 1.0 (c of a copy against a copy), all with the same rel, hence the same mmr: pool position decides.
    q = 99 + 1000
    near = feats[99] + np.float32(0.01) * feats[q]                              # a query next to the copies
    for lam in (0.3, 0.5, 0.7):
        pidx, prel = pool_expected(feats, near[None, :], [1.0], [], 60, None)
        assert set(range(99, 110)) <= set(pidx.tolist())
        got = nd.query_mean_topn_diverse(near[None, :], 40, lam, 60, return_mmr=True)
        check3(got, rerank(feats, pidx, prel, lam, 40), f"copies, lambda {lam}")
        copies = [i for i in got[0].tolist() if 99 <= i <= 109]
        assert copies == sorted(copies)                                         # whichever are picked come in row order
    c = oracle.scores(np.ascontiguousarray(feats[100:110]), np.ascontiguousarray(feats[99]))
    assert np.all(c == np.float32(1.0))
    # zero rows (10..13) score 0 against everything and tie among themselves
    got = nd.query_mean_topn_diverse(np.zeros((1, 12), np.float32), 30, 0.5, 64, return_mmr=True)
    check3(got, expected(feats, np.zeros((1, 12), np.float32), None, [], None, 0.5, 64, 30), "a zero query")
    # every rel is +0.0: pool row 0 first, then the zero rows (pen stays 0 against anything), by pool position
    assert got[0][:5].tolist() == [0, 10, 11, 12, 13]


def test_fewer_admissible_rows_than_pool_and_topn(node, engine_lib):
    nd, feats = node
    tight = {0: (0.0, 0.05), 1: (0.0, 0.2)}
    admissible = int(np.count_nonzero((feats[:, 0] <= 0.05) & (feats[:, 1] <= 0.2) & (feats[:, 0] >= 0) & (feats[:, 1] >= 0)))
    assert 0 < admissible < 256
    rows = np.array([7, 8], np.int64)
    for lam in (0.3, 1.0):
        got = nd.query_playlist_topn_diverse(rows, 256, lam, 1024, where=tight, return_mmr=True)
        check3(got, expected_rows(feats, rows, None, [], tight, lam, 1024, 256), f"tight filter, lambda {lam}")
        assert admissible - 2 <= got[0].size <= admissible
    # the raw call: count and padding -1 / 0 / 0
    from spotify_recommender_amd.engine import make_filter
    flt = make_filter(tight)
    idx, sc, mm = np.full(256, 7, np.int64), np.full(256, 7, np.float32), np.full(256, 7, np.float32)
    c = ctypes.c_int(-1)
    rc = engine_lib.mi355rec_sharded_query_playlist_topn_diverse(nd._h, rows.ctypes.data_as(ctypes.c_void_p), None, 2, None, 0, ctypes.byref(flt),
                                                                 ctypes.c_float(0.3), 1024, 256, idx.ctypes.data_as(ctypes.c_void_p),
                                                                 sc.ctypes.data_as(ctypes.c_void_p), mm.ctypes.data_as(ctypes.c_void_p),
                                                                 ctypes.byref(c))
    assert rc == 0 and c.value == got[0].size
    assert np.all(idx[c.value:] == -1) and not sc[c.value:].view(np.uint32).any() and not mm[c.value:].view(np.uint32).any()
    # out_mmr and out_score may be NULL
    rc = engine_lib.mi355rec_sharded_query_playlist_topn_diverse(nd._h, rows.ctypes.data_as(ctypes.c_void_p), None, 2, None, 0, None,
                                                                 ctypes.c_float(0.3), 40, 10, idx.ctypes.data_as(ctypes.c_void_p), None, None,
                                                                 ctypes.byref(c))
    assert rc == 0 and c.value == 10
    assert idx[:10].tolist() == expected_rows(feats, rows, None, [], None, 0.3, 40, 10)[0].tolist()


def test_diversity_lowers_the_mean_pairwise_similarity(engine_lib):
    """On a clustered catalogue the lambda = 0.3 result is less alike than the plain top-N (the oracle shows it: checked on
    the CPU for these query rows and sizes before they were written down)."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    from spotify_recommender_amd.synth import clustered_catalogue
    n, clusters = 60_000, 30
    feats = clustered_catalogue(n, 0.03, seed=4242 + clusters, clusters=clusters, contiguous=True, ramp=False, device="cpu").numpy()
    per = n // clusters
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        for q, topn, pool in ((17 * per + 5, 10, 40), (3 * per + 700, 10, 1024), (22 * per + 41, 50, 200)):
            plain = nd.query_playlist_topn([q], topn)
            got = nd.query_playlist_topn_diverse([q], topn, 0.3, pool, return_mmr=True)
            want = expected_rows(feats, [q], None, [], None, 0.3, pool, topn)
            check3(got, want, f"row {q}")
            assert mean_pairwise(feats, want[0]) < mean_pairwise(feats, plain[0]), "the oracle itself"
            assert mean_pairwise(feats, got[0]) < mean_pairwise(feats, plain[0]), (q, topn, pool)


def test_argument_errors(node, engine_lib):
    from spotify_recommender_amd import capi
    nd, feats = node
    n = feats.shape[0]
    ones2 = np.ones((2, 12), np.float32)
    bad_calls = [
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, np.nan, 40),
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, -0.1, 40),
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, 1.5, 40),
        lambda: nd.query_mean_topn_diverse(ones2, 10, np.nan, 40),
        lambda: nd.query_mean_topn_diverse(ones2, 10, -0.1, 40),
        lambda: nd.query_mean_topn_diverse(ones2, 10, 1.5, 40),
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 9),             # pool < topn
        lambda: nd.query_mean_topn_diverse(ones2, 10, 0.5, 9),
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 1025),          # pool > 1024
        lambda: nd.query_mean_topn_diverse(ones2, 10, 0.5, 1025),
        lambda: nd.query_playlist_topn_diverse([1, 2], 1025, 0.5, 1025),
        lambda: nd.query_playlist_topn_diverse([1, 2], 0, 0.5, 40),
        # inherited: weights, filter, playlist
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, weights=[1.0, np.nan]),
        lambda: nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, weights=[0.0, 0.0]),
        lambda: nd.query_mean_topn_diverse(ones2, 10, 0.5, 40, weights=[2e6, 0.0]),
        lambda: nd.query_playlist_topn_diverse([1], 10, 0.5, 40, where={1: (0.9, 0.1)}),
        lambda: nd.query_mean_topn_diverse(ones2, 10, 0.5, 40, where={1: (np.nan, 1.0)}),
        lambda: nd.query_playlist_topn_diverse(list(range(33)), 10, 0.5, 40),
        lambda: nd.query_playlist_topn_diverse([n], 10, 0.5, 40),
        lambda: nd.query_playlist_topn_diverse([1], 10, 0.5, 40, exclude=[n]),
        lambda: nd.query_playlist_topn_diverse([1], 10, 0.5, 40, exclude=list(range(1025))),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(capi.Mi355Error) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARG, i
        assert str(e.value), i
    # a bad type never reaches the library
    for bad in ("0.5", None, [0.5], True):
        with pytest.raises(ValueError):
            nd.query_playlist_topn_diverse([1, 2], 10, bad, 40)
    for bad in ("40", 40.0, [40], True):
        with pytest.raises(ValueError):
            nd.query_playlist_topn_diverse([1, 2], 10, 0.5, bad)
    with pytest.raises(ValueError):
        nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, weights=[1.0])
    # raw calls: a message in last_error that names what was wrong
    rows = np.array([1, 2], np.int64)
    idx = np.empty(16, np.int64)
    c = ctypes.c_int(0)
    for lam, pool, word in ((float("nan"), 40, b"lambda"), (-0.1, 40, b"lambda"), (1.5, 40, b"lambda"), (0.5, 9, b"pool"), (0.5, 1025, b"pool")):
        for fn, members in (("mi355rec_sharded_query_playlist_topn_diverse", rows), ("mi355rec_sharded_query_mean_topn_diverse", ones2)):
            rc = getattr(engine_lib, fn)(nd._h, members.ctypes.data_as(ctypes.c_void_p), None, 2, None, 0, None, ctypes.c_float(lam), pool, 10,
                                         idx.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(c))
            assert rc == capi.ERR_INVALID_ARG
            assert word in engine_lib.mi355rec_sharded_last_error(nd._h)
    # the edges are allowed: lambda 0 and 1, pool == topn, pool 1024
    for lam, pool in ((0.0, 10), (1.0, 10), (0.5, 1024)):
        check3(nd.query_playlist_topn_diverse([1, 2], 10, lam, pool, return_mmr=True), expected_rows(feats, [1, 2], None, [], None, lam, pool, 10),
               f"edge {lam} {pool}")
    # a good call after the errors still answers
    check3(nd.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, weights=[1.0, -0.5], return_mmr=True),
           expected_rows(feats, [1, 2], [1.0, -0.5], [], None, 0.5, 40, 10), "after errors")


# ---- the C++ drop-in (through its shim) and the CLI ---------------------------------------------------------------------
def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _shim():
    from tests.test_weighted_cpu import _shim as weighted_shim
    shim = weighted_shim()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    shim.shim_recommend_diverse.restype = ctypes.c_int64
    shim.shim_recommend_diverse.argtypes = [P, I, I, F, I, P, P, P, I, P, P, ctypes.c_int64]
    shim.shim_recommend_for_playlist_diverse.restype = ctypes.c_int64
    shim.shim_recommend_for_playlist_diverse.argtypes = [P, P, I, P, I, I, P, P, P, I, P, I, F, I, P, P, ctypes.c_int64]
    return shim


@pytest.fixture()
def sample(engine_lib, tmp_path):
    from tests.test_playlist_cpu import _write_csv
    from tests.test_weighted_cpu import _served_matrix
    shim = _shim()
    _write_csv(tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    feats = _served_matrix(shim, tmp_path / "songs_data.bin")
    track_ids = [l.split(",", 1)[0] for l in (tmp_path / "songs.csv").read_text().splitlines()[1:]]
    return shim, feats, track_ids, tmp_path


def _ids(stdout):
    return [l.split("ID:", 1)[1].strip() for l in stdout.split("Recommendations:", 1)[1].splitlines() if l.strip().startswith("ID:")]


def test_cli_diverse_and_pool(sample):
    shim, feats, t, cwd = sample
    assert feats.shape[0] > 45
    # --id
    p = _run(["--id", t[4], "--diverse", "0.5", "--pool", "40", "-n", "5"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in expected_rows(feats, [4], None, [], None, 0.5, 40, 5)[0]], p.stdout
    # --playlist ... --dislike ...
    liked, disliked = [0, 3, 6], [9, 12]
    lk, dl = ",".join(t[i] for i in liked), ",".join(t[i] for i in disliked)
    p = _run(["--playlist", lk, "--dislike", dl, "--diverse", "0.5", "--pool", "40", "-n", "5"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in expected_rows(feats, liked + disliked, [1, 1, 1, -0.5, -0.5], [], None, 0.5, 40, 5)[0]], p.stdout
    # --where (and the default pool: 4 x N)
    where = {"energy": (0.0, 0.9)}
    p = _run(["--id", t[4], "--where", "energy=0:0.9", "--diverse", "0.5", "--pool", "40", "-n", "5"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in expected_rows(feats, [4], None, [], where, 0.5, 40, 5)[0]], p.stdout
    p = _run(["--playlist", lk, "--weights", "2,0.5,1", "--where", "energy=0:0.9", "--diverse", "0.3", "-n", "5"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in expected_rows(feats, liked, [2, 0.5, 1], [], where, 0.3, 20, 5)[0]], p.stdout
    # lambda = 1 is the plain result
    assert _ids(_run(["--id", t[4], "--diverse", "1", "-n", "5"], cwd).stdout) == _ids(_run(["--id", t[4], "-n", "5"], cwd).stdout)
    # the refusals: exit status 1 and a message
    for bad, msg in ((["--diverse", "1.5"], "--diverse"), (["--diverse", "-0.1"], "--diverse"), (["--diverse", "nan"], "--diverse"),
                     (["--diverse", "x"], "--diverse"), (["--diverse"], "needs a value"),
                     (["--diverse", "0.5", "--pool", "1025"], "--pool"), (["--diverse", "0.5", "--pool", "0"], "--pool"),
                     (["--diverse", "0.5", "--pool", "4", "-n", "5"], "--pool"), (["--pool", "40"], "--pool"),
                     (["--diverse", "0.5", "--genre", "pop"], "--genre")):
        p = _run(["--id", t[4], *bad], cwd)
        assert p.returncode == 1, (bad, p.stdout)
        assert msg in p.stderr, (bad, p.stderr)
    p = _run(["--playlist", lk, "--diverse", "2"], cwd)
    assert p.returncode == 1 and "--diverse" in p.stderr
    usage = _run([], cwd).stdout
    assert "--diverse" in usage and "--pool" in usage


def test_recommender_diverse_through_the_shim(sample):
    shim, feats, t, cwd = sample
    h = shim.shim_load(str(cwd / "songs_data.bin").encode())
    assert h
    try:
        assert shim.shim_initialize(h) == 1

        def arrays(ranges, exclude):
            f = np.array([r[0] for r in ranges] or [0], np.int32)
            lo = np.array([r[1] for r in ranges] or [0], np.float32)
            hi = np.array([r[2] for r in ranges] or [0], np.float32)
            return f, lo, hi, np.array(list(exclude) or [0], np.int32)

        def diverse(song, topn, lam, pool=0, ranges=()):
            f, lo, hi, _ = arrays(ranges, ())
            out, sc = np.full(64, -7, np.int32), np.zeros(64, np.float32)
            n = shim.shim_recommend_diverse(h, song, topn, lam, pool, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, len(ranges),
                                            out.ctypes.data, sc.ctypes.data, 64)
            return out[:max(n, 0)].astype(np.int64), sc[:max(n, 0)]

        def playlist(songs, weights, topn, lam, pool=0, ranges=(), exclude=()):
            s, w = np.array(songs, np.int32), np.array(list(weights) or [0], np.float32)
            f, lo, hi, ex = arrays(ranges, exclude)
            out, sc = np.full(64, -7, np.int32), np.zeros(64, np.float32)
            n = shim.shim_recommend_for_playlist_diverse(h, s.ctypes.data, len(songs), w.ctypes.data, len(weights), topn, f.ctypes.data,
                                                         lo.ctypes.data, hi.ctypes.data, len(ranges), ex.ctypes.data, len(exclude), lam, pool,
                                                         out.ctypes.data, sc.ctypes.data, 64)
            return out[:max(n, 0)].astype(np.int64), sc[:max(n, 0)]

        # lastScores() holds the relevance
        check(diverse(4, 10, 0.5, 40), expected_rows(feats, [4], None, [], None, 0.5, 40, 10)[:2], "recommendDiverse")
        check(diverse(4, 10, 0.7), expected_rows(feats, [4], None, [], None, 0.7, 40, 10)[:2], "the default pool")
        check(diverse(4, 5, 0.3, 20, [(1, 0.0, 0.8)]), expected_rows(feats, [4], None, [], {1: (0.0, 0.8)}, 0.3, 20, 5)[:2], "filtered")
        w = [1.0, -0.75, 0.25]
        check(playlist([0, 3, 5], w, 10, 0.5, 40, [(1, 0.0, 0.8)], [1, 2]),
              expected_rows(feats, [0, 3, 5], w, [1, 2], {1: (0.0, 0.8)}, 0.5, 40, 10)[:2], "playlist, weighted, filtered, excluded")
        check(playlist([0, 3], [], 10, 0.5), expected_rows(feats, [0, 3], None, [], None, 0.5, 40, 10)[:2], "playlist without weights")
        # bad input: {} (and a message on stderr)
        assert diverse(4, 10, float("nan"))[0].size == 0
        assert diverse(4, 10, -0.1)[0].size == 0
        assert diverse(4, 10, 1.5)[0].size == 0
        assert diverse(4, 10, 0.5, 9)[0].size == 0
        assert diverse(4, 10, 0.5, 1025)[0].size == 0
        assert diverse(4, 10, 0.5, -1)[0].size == 0
        assert diverse(-1, 10, 0.5)[0].size == 0
        assert playlist([0, 3], [1.0], 10, 0.5)[0].size == 0                    # the wrong length
        assert playlist([0, 3], [0.0, 0.0], 10, 0.5)[0].size == 0
        check(diverse(4, 10, 0.5, 40), expected_rows(feats, [4], None, [], None, 0.5, 40, 10)[:2], "after the refusals")
    finally:
        shim.shim_free(h)
