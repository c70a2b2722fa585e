"""LABELS on a host without a GPU: label-filtered top-N through the node handle (served by the product's CPU backend,
csrc/cpu_backend.cpp), the C-ABI's argument errors, and the drop-in CLI's --genre.  Checked against the oracle: scores
restricted to the selected rows, canonical order, bit-equal scores and identical ids."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import catalogue, check, expected


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

SETS = {
    "one": [7],
    "two": [3, 5],
    "alternating": list(range(0, 114, 2)),
    "all": list(range(114)),
    "empty label": [500],
    "duplicates": [5, 5, 3, 5],
}


@pytest.fixture(scope="module")
def node(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, labels = catalogue(20_000, 114, seed=11)
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(labels)
        yield nd, feats, labels


@pytest.mark.parametrize("name", sorted(SETS))
def test_filtered_queries_match_the_oracle(node, name):
    nd, feats, labels = node
    wanted = SETS[name]
    selected = int(np.isin(labels, wanted).sum())
    # query rows: inside the set (a tie row, a zero row where the set has them), and outside it
    inside = [r for r in (99, 10, 200) if labels[r] in wanted] or [int(np.flatnonzero(np.isin(labels, wanted))[0])] if selected else []
    outside = [int(np.flatnonzero(~np.isin(labels, wanted))[0]), 19_999]
    for q in inside + outside:
        for topn in (1, 10, 100, selected + 5):
            want = expected(feats, labels, feats[q], q, wanted, topn)
            check(nd.query_row_topn_labels(q, wanted, topn), want, f"{name} row {q} top-{topn}")
            assert len(want[0]) == min(topn, selected - int(labels[q] in wanted))
    vec = np.random.default_rng(5).random(12, dtype=np.float32)
    for excl in (-1, outside[0]):
        check(nd.query_topn_labels(vec, excl, wanted, 50), expected(feats, labels, vec, excl, wanted, 50), f"{name} by value")


def test_ties_and_zero_rows_keep_the_canonical_order(node):
    nd, feats, labels = node
    idx, sc = nd.query_row_topn_labels(99, [5], 20)
    dup = [r for r in range(100, 110)]
    assert idx[:10].tolist() == dup, idx          # the ten exact copies of row 99: score 1.0 each, rows ascending
    idx, sc = nd.query_row_topn_labels(10, [3], 1000)   # a zero query: every score is 0, rows ascending
    want = np.flatnonzero(labels == 3)
    assert idx.tolist() == [int(r) for r in want if r != 10] and not sc.any()


def test_argument_errors(node, engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd, feats, labels = node
    for bad in ([], [1024], [-2], [3, 1024]):
        with pytest.raises(capi.Mi355Error) as e:
            nd.query_row_topn_labels(0, bad, 10)
        assert e.value.code == capi.ERR_INVALID_ARG
    # the raw call with n_labels = 0 and a message in last_error
    L = engine_lib
    idx = np.empty(4, np.int64)
    lab = np.array([1], np.int32)
    cnt = ctypes.c_int(0)
    rc = L.mi355rec_sharded_query_row_topn_labels(nd._h, 0, lab.ctypes.data_as(ctypes.c_void_p), 0, 4,
                                                  idx.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(cnt))
    assert rc == capi.ERR_INVALID_ARG and L.mi355rec_sharded_last_error(nd._h)
    # labels never set
    with NodeEngine(feats[:100], placement=capi.PLACEMENT_AUTO) as fresh:
        with pytest.raises(capi.Mi355Error, match="no labels"):
            fresh.query_row_topn_labels(0, [1], 5)
        with pytest.raises(capi.Mi355Error):
            fresh.set_labels(labels[:99])          # one label per row
        with pytest.raises(capi.Mi355Error):
            fresh.set_labels(np.full(100, 1024, np.int32))
        fresh.set_labels(labels[:100])
        fresh.set_labels(None)                   # dropped again
        with pytest.raises(capi.Mi355Error, match="no labels"):
            fresh.query_topn_labels(feats[0], -1, [1], 5)


def test_unfiltered_queries_are_unchanged_by_labels(node):
    nd, feats, labels = node
    for q in (0, 99, 12_345):
        want = oracle.topn_canonical(oracle.scores(feats, feats[q]), q, 10)
        idx, sc = nd.query_row_topn(q, 10)
        assert idx.tolist() == want[0].tolist() and np.array_equal(sc, want[1] + np.float32(0))


# ---- the drop-in CLI ------------------------------------------------------------------------------------------------
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


def test_cli_genre_restricted_recommendations(engine_lib, tmp_path):
    from spotify_recommender_amd import build
    build.build_shim()
    _write_csv(tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    # the matrix and genres the CLI serves, read back through the shim (what the CLI itself loads)
    shim = ctypes.CDLL(str(build.LIB_SHIM))
    shim.shim_load.restype = ctypes.c_void_p
    shim.shim_load.argtypes = [ctypes.c_char_p]
    shim.shim_free.argtypes = [ctypes.c_void_p]
    shim.shim_song_count.restype = ctypes.c_int64
    shim.shim_song_count.argtypes = [ctypes.c_void_p]
    shim.shim_song_features.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    shim.shim_genre_name.restype = ctypes.c_int64
    shim.shim_genre_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
    h = shim.shim_load(str(tmp_path / "songs_data.bin").encode())
    assert h
    try:
        n = shim.shim_song_count(h)
        feats = np.zeros((n, 12), np.float32)
        gid = np.zeros(n, np.int32)
        g = ctypes.c_int(0)
        for i in range(n):
            shim.shim_song_features(h, i, feats[i].ctypes.data, ctypes.byref(g))
            gid[i] = g.value
        buf = ctypes.create_string_buffer(64)
        names = {}
        for i in set(gid.tolist()):
            k = shim.shim_genre_name(h, int(i), buf, 64)
            names[buf.raw[:k].decode()] = int(i)
    finally:
        shim.shim_free(h)
    q = 123
    for genre in ("jazz", "Rock"):
        p = _run(["--id", f"t{q:04d}", "-n", "5", "--genre", genre], tmp_path)
        assert p.returncode == 0, p.stdout + p.stderr
        out = p.stdout.split("Recommendations:", 1)[1]
        printed = [l.split("Genre:", 1)[1].strip() for l in out.splitlines() if "Genre:" in l]
        assert printed == [genre.lower()] * 5, p.stdout
        ids = [int(l.split("t", 1)[1]) for l in out.splitlines() if l.strip().startswith("ID:")]
        want, _ = expected(feats, gid, feats[q], q, [names[genre.lower()]], 5)
        assert ids == want.tolist(), (ids, want)
    # two genres at once
    p = _run(["--song", "Song 0200", "-n", "8", "--genre", "pop", "--genre", "metal"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.split("Recommendations:", 1)[1]
    assert {l.split("Genre:", 1)[1].strip() for l in out.splitlines() if "Genre:" in l} <= {"pop", "metal"}
    # an unknown genre is an error
    p = _run(["--id", f"t{q:04d}", "--genre", "polka"], tmp_path)
    assert p.returncode == 1 and "Unknown genre" in p.stderr
    # without --genre: the unfiltered recommendations, as before
    p = _run(["--id", f"t{q:04d}", "-n", "5"], tmp_path)
    assert p.returncode == 0
    out = p.stdout.split("Recommendations:", 1)[1]
    ids = [int(l.split("t", 1)[1]) for l in out.splitlines() if l.strip().startswith("ID:")]
    assert ids == oracle.topn_canonical(oracle.scores(feats, feats[q]), q, 5)[0].tolist()
    assert "Restricted to genres" not in p.stdout
