"""PLAYLISTS on a host without a GPU: the top-N by mean score against up to 32 songs through the node handle (served by the
product's CPU backend, csrc/cpu_backend.cpp), the C-ABI's argument errors, and the drop-in CLI's --playlist.  Checked
against the oracle (tests/playlist_oracle.py): identical ids, bit-equal scores."""
import ctypes
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import catalogue, check
from tests.playlist_oracle import expected, expected_rows


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")


@pytest.fixture(scope="module")
def node(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, _ = catalogue(20_000, 114, seed=11)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        yield nd, feats


@pytest.mark.parametrize("k", [1, 2, 7, 32])
@pytest.mark.parametrize("topn", [1, 10, 1024])
def test_playlists_match_the_oracle(node, k, topn):
    nd, feats = node
    rng = np.random.default_rng(k * 1000 + topn)
    rows = rng.choice(feats.shape[0], size=k, replace=False)
    check(nd.query_playlist_topn(rows, topn), expected_rows(feats, rows, [], topn), f"k={k} top-{topn} by row")
    vecs = rng.random((k, 12), dtype=np.float32)
    check(nd.query_mean_topn(vecs, topn), expected(feats, vecs, [], topn), f"k={k} top-{topn} by value")
    excl = rng.integers(0, feats.shape[0], size=300)
    check(nd.query_mean_topn(vecs, topn, excl), expected(feats, vecs, excl, topn), f"k={k} top-{topn} excluded")


def test_one_song_playlist_is_the_single_query(node):
    nd, feats = node
    for q in (0, 99, 10, 12_345):
        for topn in (1, 10, 500):
            got = nd.query_playlist_topn([q], topn)
            want = nd.query_row_topn(q, topn)
            assert got[0].tolist() == want[0].tolist(), q
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), q
            check(got, expected_rows(feats, [q], [], topn), f"row {q}")


def test_duplicate_and_zero_members(node):
    nd, feats = node
    # duplicates count with their multiplicity: (a, a, b) weighs a twice
    a, b = 5, 777
    want = expected_rows(feats, [a, a, b], [], 50)
    check(nd.query_playlist_topn([a, a, b], 50), want, "duplicates")
    assert nd.query_playlist_topn([a, b], 50)[0].tolist() != want[0].tolist()
    # zero rows (10..13 of the catalogue) score 0 against everything: a member that is one only scales the others' mean
    check(nd.query_playlist_topn([10, a], 40), expected_rows(feats, [10, a], [], 40), "a zero member")
    check(nd.query_playlist_topn([10, 11], 40), expected_rows(feats, [10, 11], [], 40), "zero members only")
    zero = np.zeros((3, 12), np.float32)
    idx, sc = nd.query_mean_topn(zero, 25)
    assert idx.tolist() == list(range(25)) and not sc.any()        # every score 0: rows ascending


def test_exclusion_lists_with_duplicates(node):
    nd, feats = node
    top = expected_rows(feats, [99], [], 40)[0]
    excl = [int(top[0]), int(top[0]), int(top[3]), 19_999, int(top[3])]
    want = expected_rows(feats, [99], excl, 30)
    got = nd.query_playlist_topn([99], 30, excl)
    check(got, want, "duplicated exclusions")
    assert not set(got[0].tolist()) & set(excl)
    # members named in the caller's list too, and the list at its limit
    big = list(range(1000, 2023)) + [99]
    check(nd.query_playlist_topn([99, 1500], 100, big), expected_rows(feats, [99, 1500], big, 100), "1024 ids")


def test_ties_zero_and_duplicate_rows_keep_the_canonical_order(node):
    nd, feats = node
    # rows 100..109 are copies of 99 and 200..204 scaled copies: a playlist of copies ranks the rest by row
    idx, sc = nd.query_playlist_topn([99, 100], 20)
    assert idx[:9].tolist() == list(range(101, 110)), idx       # the other copies: score 1.0 each, rows ascending
    check((idx, sc), expected_rows(feats, [99, 100], [], 20), "copies")


def test_count_is_what_is_left(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = oracle.mt19937_uniform(3, 40)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        idx, sc = nd.query_playlist_topn([0, 1, 1], 100, [5, 5, 39])
        assert len(idx) == 40 - 4
        check((idx, sc), expected_rows(feats, [0, 1, 1], [5, 39], 100), "small")
        assert len(nd.query_playlist_topn([0], 10, list(range(1, 40)))[0]) == 0


def test_argument_errors(node, engine_lib):
    from spotify_recommender_amd import capi
    nd, feats = node
    n = feats.shape[0]
    bad_calls = [
        lambda: nd.query_playlist_topn([], 10),
        lambda: nd.query_playlist_topn(list(range(33)), 10),
        lambda: nd.query_mean_topn(np.ones((33, 12), np.float32), 10),
        lambda: nd.query_playlist_topn([1], 0),
        lambda: nd.query_playlist_topn([1], -3),
        lambda: nd.query_playlist_topn([1], 1025),
        lambda: nd.query_playlist_topn([n], 10),
        lambda: nd.query_playlist_topn([-1], 10),
        lambda: nd.query_playlist_topn([1], 10, [n]),
        lambda: nd.query_mean_topn(np.ones((2, 12), np.float32), 10, [-1]),
        lambda: nd.query_playlist_topn([1], 10, list(range(1025))),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(capi.Mi355Error) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARG, i
    # raw calls: a NULL list with n_exclude > 0, n_exclude < 0; a message in last_error
    L = engine_lib
    rows = np.array([1, 2], np.int64)
    idx = np.empty(10, np.int64)
    sc = np.empty(10, np.float32)
    c = ctypes.c_int(0)
    for excl, n_ex in ((None, 3), (None, -1)):
        rc = L.mi355rec_sharded_query_playlist_topn(nd._h, rows.ctypes.data_as(ctypes.c_void_p), 2, excl, n_ex, 10,
                                                    idx.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p),
                                                    ctypes.byref(c))
        assert rc == capi.ERR_INVALID_ARG
        assert L.mi355rec_sharded_last_error(nd._h)
    # a good call after the errors still answers
    check(nd.query_playlist_topn([1, 2], 10), expected_rows(feats, [1, 2], [], 10), "after errors")


GENRES = ["rock", "indie", "jazz", "pop", "metal"]


def _write_csv(path, rows=600, seed=4):
    rng = np.random.default_rng(seed)
    lines = ["track_id,track_name,artists,danceability,energy,key,loudness,mode,speechiness,acousticness,"
             "instrumentalness,liveness,valence,tempo,track_genre"]
    for i in range(rows):
        r = rng.random(10)
        lines.append(f"t{i:04d},Song {i:04d},Artist {i % 37},{r[0]:.3f},{r[1]:.3f},{int(r[2] * 11)},{-60 * r[3]:.3f},"
                     f"{int(r[4] * 2)},{r[5]:.4f},{r[6]:.5f},{r[7] ** 6:.6f},{r[8]:.4f},{r[9]:.4f},{60 + 140 * r[2]:.3f},"
                     f"{GENRES[(i // 40) % len(GENRES)]}")
    path.write_text("\n".join(lines) + "\n")


def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _served_matrix(path):
    from spotify_recommender_amd import build
    shim = ctypes.CDLL(str(build.LIB_SHIM))
    shim.shim_load.restype = ctypes.c_void_p
    shim.shim_load.argtypes = [ctypes.c_char_p]
    shim.shim_free.argtypes = [ctypes.c_void_p]
    shim.shim_song_count.restype = ctypes.c_int64
    shim.shim_song_count.argtypes = [ctypes.c_void_p]
    shim.shim_song_features.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
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


def test_cli_playlist_recommendations(engine_lib, tmp_path):
    from spotify_recommender_amd import build
    build.build_shim()
    _write_csv(tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    feats = _served_matrix(tmp_path / "songs_data.bin")
    members = [123, 7, 450]
    p = _run(["--playlist", ",".join(f"t{m:04d}" for m in members), "-n", "6"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    head, out = p.stdout.split("Recommendations:", 1)
    listed = [l.split('"')[1] for l in head.splitlines() if l.strip()[:1].isdigit() and '"' in l]
    assert listed == [f"Song {m:04d}" for m in members], p.stdout
    ids = [int(l.split("t", 1)[1]) for l in out.splitlines() if l.strip().startswith("ID:")]
    want, _ = expected_rows(feats, members, [], 6)
    assert ids == want.tolist(), (ids, want)
    assert "Recommendation complete!" in p.stdout
    # an unknown id: an error and exit status 1
    p = _run(["--playlist", "t0001,nosuchid"], tmp_path)
    assert p.returncode == 1
    assert "nosuchid" in p.stderr
