"""ROW SETS through the C++ drop-in and the CLI (include/Recommender.h: setRowSet / clearRowSet; csrc/main.cpp: --seen FILE and
--only FILE), on tests/golden/sample_songs_data.bin and on a 600-song catalogue: a small set against recommendForPlaylist with the
same ids appended to alsoExclude (--only: the ids NOT listed appended), beside --where, --metric euclidean, --scale, --diverse and
--genre; both flags together (refused), a file with unknown ids (skipped, counted on stderr), an unreadable file (exit 1)."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest


def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _ids(stdout):
    return [l.split("ID:", 1)[1].strip() for l in stdout.split("Recommendations:", 1)[1].splitlines() if l.strip().startswith("ID:")]


class Shim:
    """The Recommender class over one songs_data.bin, through csrc/shim_capi.cpp."""

    def __init__(self, path):
        from spotify_recommender_amd import build
        build.build_shim()
        L = self.L = ctypes.CDLL(str(build.LIB_SHIM))
        P, I = ctypes.c_void_p, ctypes.c_int
        L.shim_load.restype = P
        L.shim_load.argtypes = [ctypes.c_char_p]
        L.shim_free.argtypes = [P]
        L.shim_initialize.argtypes = [P]
        L.shim_song_count.restype = ctypes.c_int64
        L.shim_song_count.argtypes = [P]
        L.shim_song_string.restype = ctypes.c_int64
        L.shim_song_string.argtypes = [P, ctypes.c_int64, I, ctypes.c_char_p, ctypes.c_int64]
        L.shim_set_row_set.argtypes = [P, P, I, I]
        L.shim_recommend_for_playlist.restype = ctypes.c_int64
        L.shim_recommend_for_playlist.argtypes = [P, P, I, I, P, I, P, P, ctypes.c_int64]
        L.shim_recommend_for_playlist_where.restype = ctypes.c_int64
        L.shim_recommend_for_playlist_where.argtypes = [P, P, I, I, P, P, P, I, P, I, P, P, ctypes.c_int64]
        L.shim_recommend_by_index.restype = ctypes.c_int64
        L.shim_recommend_by_index.argtypes = [P, I, I, P, P, ctypes.c_int64]
        self.h = L.shim_load(str(path).encode())
        assert self.h and L.shim_initialize(self.h) == 1
        self.n = int(L.shim_song_count(self.h))
        buf = ctypes.create_string_buffer(256)
        self.track_ids = []
        for i in range(self.n):
            size = L.shim_song_string(self.h, i, 0, buf, 256)
            self.track_ids.append(buf.raw[:size].decode())

    def close(self):
        self.L.shim_free(self.h)

    def set_rows(self, rows, only=False):
        a = np.asarray(list(rows) or [0], np.int32)
        return self.L.shim_set_row_set(self.h, a.ctypes.data, len(rows), int(only))

    def clear(self):
        assert self.L.shim_set_row_set(self.h, None, -1, 0) == 1

    def playlist(self, songs, topn, exclude=(), where=None):
        s, ex = np.asarray(songs, np.int32), np.asarray(list(exclude) or [0], np.int32)
        out, sc = np.full(1024, -7, np.int32), np.zeros(1024, np.float32)
        if where is None:
            n = self.L.shim_recommend_for_playlist(self.h, s.ctypes.data, len(songs), topn, ex.ctypes.data, len(exclude), out.ctypes.data,
                                                   sc.ctypes.data, 1024)
        else:
            f, lo, hi = np.asarray([where[0]], np.int32), np.asarray([where[1]], np.float32), np.asarray([where[2]], np.float32)
            n = self.L.shim_recommend_for_playlist_where(self.h, s.ctypes.data, len(songs), topn, f.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                                         1, ex.ctypes.data, len(exclude), out.ctypes.data, sc.ctypes.data, 1024)
        return out[:n].tolist(), sc[:n].copy()

    def by_index(self, song, topn):
        out, sc = np.full(1024, -7, np.int32), np.zeros(1024, np.float32)
        n = self.L.shim_recommend_by_index(self.h, song, topn, out.ctypes.data, sc.ctypes.data, 1024)
        return out[:n].tolist(), sc[:n].copy()


@pytest.fixture()
def golden(engine_lib, golden_dir, tmp_path):
    shutil.copy(golden_dir / "sample_songs_data.bin", tmp_path / "songs_data.bin")
    shim = Shim(tmp_path / "songs_data.bin")
    yield shim, tmp_path
    shim.close()


@pytest.fixture()
def catalogue(engine_lib, tmp_path):
    from tests.test_playlist_cpu import _write_csv
    from spotify_recommender_amd import build
    build.build_shim()
    _write_csv(tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    shim = Shim(tmp_path / "songs_data.bin")
    yield shim, tmp_path
    shim.close()


def _same(a, b):
    assert a[0] == b[0] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (a, b)


def test_recommender_row_set_on_the_golden_sample(golden):
    shim, _ = golden
    assert shim.n == 4
    for members in ([0], [1, 2]):
        for seen in ([], [3], [0, 3], [1, 1, 2], [0, 1, 2, 3]):
            want = shim.playlist(members, 4, exclude=seen) if len(set(seen) | set(members)) < 4 else ([], np.zeros(0, np.float32))
            assert shim.set_rows(seen) == 1
            _same(shim.playlist(members, 4), want)
            rest = [i for i in range(4) if i not in seen]
            assert shim.set_rows(rest, only=True) == 1
            _same(shim.playlist(members, 4), want)
            shim.clear()
            _same(shim.playlist(members, 4), shim.playlist(members, 4, exclude=[]))
    assert shim.set_rows([1]) == 1
    assert shim.set_rows([1, 4]) == 0                             # refused: the set stays as it was
    assert shim.set_rows([-1]) == 0
    got = shim.playlist([0], 4)
    shim.clear()
    _same(got, shim.playlist([0], 4, exclude=[1]))


def test_recommender_row_set(catalogue):
    shim, _ = catalogue
    n = shim.n
    rng = np.random.default_rng(3)
    seen = sorted(int(i) for i in rng.choice(n, size=300, replace=False))
    members = [5, 70, 333]
    plain = shim.by_index(7, 10)
    want = shim.playlist(members, 50, exclude=seen)
    want_w = shim.playlist(members, 50, exclude=seen, where=(1, 0.2, 0.9))
    assert shim.set_rows(seen + seen[:5]) == 1
    _same(shim.playlist(members, 50), want)
    _same(shim.playlist(members, 50, exclude=seen[:10]), want)     # beside alsoExclude
    _same(shim.playlist(members, 50, where=(1, 0.2, 0.9)), want_w)
    _same(shim.by_index(7, 10), plain)                            # the reference's single-query path is unchanged
    assert shim.set_rows([i for i in range(n) if i not in seen], only=True) == 1
    _same(shim.playlist(members, 50), want)
    _same(shim.by_index(7, 10), plain)
    big = list(range(0, n, 2)) * 4                                # 1200 ids: beyond alsoExclude's 1024
    assert shim.set_rows(big) == 1
    got = shim.playlist(members, 50)
    assert len(got[0]) == 50 and all(i % 2 == 1 for i in got[0])
    shim.clear()
    _same(shim.playlist(members, 50, exclude=seen), want)


def test_cli_on_the_golden_sample(golden):
    shim, cwd = golden
    t = shim.track_ids
    (cwd / "seen.txt").write_text(f"{t[3]}\n\n  {t[3]}  \nno-such-track\n")
    p = _run(["--playlist", t[0], "--seen", "seen.txt", "-n", "4"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[i] for i in shim.playlist([0], 4, exclude=[3])[0]]
    assert "2 tracks, 1 lines skipped" in p.stderr
    p = _run(["--id", t[0], "--only", "seen.txt", "-n", "4"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == [t[3]]


def test_cli(catalogue):
    shim, cwd = catalogue
    t, n = shim.track_ids, shim.n
    rng = np.random.default_rng(5)
    seen = sorted(int(i) for i in rng.choice(n, size=200, replace=False))
    rest = [i for i in range(n) if i not in seen]
    (cwd / "seen.txt").write_text("\n".join([t[i] for i in seen] + ["unknown-a", "unknown-b", "", t[seen[0]]]) + "\n")
    (cwd / "only.txt").write_text("\n".join(t[i] for i in rest) + "\n")
    members = [5, 70, 333]
    lk = ",".join(t[i] for i in members)
    want = [t[i] for i in shim.playlist(members, 8, exclude=seen)[0]]
    p = _run(["--playlist", lk, "--seen", "seen.txt", "-n", "8"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    assert _ids(p.stdout) == want, p.stdout
    assert "201 tracks, 2 lines skipped" in p.stderr and "Leaving out 201 listed songs" in p.stdout
    p = _run(["--playlist", lk, "--only", "only.txt", "-n", "8"], cwd)
    assert p.returncode == 0 and _ids(p.stdout) == want, p.stdout + p.stderr
    assert "0 lines skipped" in p.stderr
    # the one-song playlist of --id and --song
    one = [t[i] for i in shim.playlist([7], 6, exclude=seen)[0]]
    for mode, query in (("--id", t[7]), ("--song", "Song 0007")):
        p = _run([mode, query, "--seen", "seen.txt", "-n", "6"], cwd)
        assert p.returncode == 0 and _ids(p.stdout) == one, p.stdout + p.stderr
    # beside the options those modes already take
    p = _run(["--playlist", lk, "--seen", "seen.txt", "--where", "energy=0.2:0.9", "-n", "8"], cwd)
    assert p.returncode == 0 and _ids(p.stdout) == [t[i] for i in shim.playlist(members, 8, exclude=seen, where=(1, 0.2, 0.9))[0]], p.stdout + p.stderr
    seen_set = set(t[i] for i in seen)
    for more in (["--metric", "euclidean"], ["--scale", "key=0", "--scale", "tempo=2"], ["--metric", "euclidean", "--scale", "mode=0"],
                 ["--diverse", "0.5"], ["--max-per-artist", "1"], ["--genre", "rock"], ["--dislike", t[9]]):
        a = _run(["--playlist", lk, "--seen", "seen.txt", "-n", "8", *more], cwd)
        b = _run(["--playlist", lk, "--only", "only.txt", "-n", "8", *more], cwd)
        assert a.returncode == 0 and b.returncode == 0, (more, a.stderr, b.stderr)
        assert _ids(a.stdout) == _ids(b.stdout) and len(_ids(a.stdout)) == 8 and not seen_set & set(_ids(a.stdout)), (more, a.stdout)
        assert _ids(a.stdout) != _ids(_run(["--playlist", lk, "-n", "8", *more], cwd).stdout) or not seen_set & set(_ids(a.stdout))
    # refusals: exit status 1 and a message
    for bad, msg in ((["--seen", "seen.txt", "--only", "only.txt"], "cannot be combined"), (["--seen", "seen.txt", "--seen", "seen.txt"], "once"),
                     (["--seen", "missing.txt"], "cannot open the row set file 'missing.txt'"), (["--only"], "needs a file")):
        p = _run(["--playlist", lk, *bad], cwd)
        assert p.returncode == 1 and msg in p.stderr, (bad, p.stdout, p.stderr)
    p = _run(["--id", t[7], "--seen", "seen.txt", "--genre", "rock"], cwd)
    assert p.returncode == 1 and "--playlist <one id>" in p.stderr
    (cwd / "everything.txt").write_text("\n".join(t) + "\n")
    p = _run(["--playlist", lk, "--seen", "everything.txt"], cwd)
    assert p.returncode == 1 and "No recommendations found" in p.stderr
    assert "--seen FILE" in _run([], cwd).stdout
