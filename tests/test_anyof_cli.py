"""ANY-OF REQUESTS through the C++ drop-in and the CLI (include/Recommender.h: Query::anyOf, lastMatchedSongs; csrc/main.cpp:
--match any), on tests/golden/sample_songs_data.bin and on a 600-song catalogue: the recommendations and the matched-track column
against the host merge of one-member playlist requests (the max per song, the first member that attains it), beside --where, --seen,
--only and --genre; every refusal with its message; --match mean equal to no option."""
import ctypes
import re

import numpy as np

from tests.test_rowset_cli import Shim, _ids, _run, catalogue, golden  # noqa: F401  (catalogue, golden: the fixtures)

REFUSED = (["--weights", "1,1,1"], ["--dislike", "X"], ["--dislike-weight", "0.5"], ["--diverse", "0.5"], ["--pool", "50"],
           ["--max-per-artist", "1"], ["--priors", "priors.txt"], ["--prior-weight", "0.5"], ["--scale", "key=0"],
           ["--candidates", "list.txt"], ["--score", "list.txt"])


def _matches(stdout):
    """The matched-track column of the recommendations, in order."""
    return re.findall(r'^\d+\. ".*"  \(matches "(.*)"\)$', stdout.split("Recommendations:", 1)[1], flags=re.M)


def _name(shim, i):
    buf = ctypes.create_string_buffer(512)
    size = shim.L.shim_song_string(shim.h, i, 1, buf, 512)
    return buf.raw[:size].decode()


def _anyof(shim, songs, topn, exclude=(), where=None, refuse=0):
    fn = shim.L.shim_query_anyof
    fn.restype = ctypes.c_int64
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fn.argtypes = [P, P, I, P, I, I, F, F, I, I, P, P, P, ctypes.c_int64]
    s, ex = np.asarray(songs, np.int32), np.asarray(list(exclude) or [0], np.int32)
    out, sc, m = np.full(1024, -7, np.int32), np.zeros(1024, np.float32), np.full(1024, -7, np.int32)
    f, lo, hi = where if where is not None else (-1, 0.0, 0.0)
    n = fn(shim.h, s.ctypes.data, len(songs), ex.ctypes.data, len(exclude), f, lo, hi, topn, refuse, out.ctypes.data, sc.ctypes.data,
           m.ctypes.data, 1024)
    assert n >= 0
    return out[:n].tolist(), sc[:n].copy(), m[:n].tolist()


def _merged(shim, songs, topn, exclude=(), where=None):
    """What a caller had to do before: one playlist request per song with the whole exclusion list, the max per song."""
    best = {}
    for s in songs:
        ids, sc = shim.playlist([s], topn, exclude=list(exclude) + list(songs), where=where)
        for i, v in zip(ids, sc.tolist()):
            if i not in best or v > best[i][0]:
                best[i] = (v, s)                                  # (songs in order and a strict compare: the first that attains it)
    order = sorted(best, key=lambda i: (-best[i][0], i))[:topn]
    return order, np.asarray([best[i][0] for i in order], np.float32), [best[i][1] for i in order]


def _check(got, want):
    assert got[0] == want[0] and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and got[2] == want[2], (got, want)


def test_recommender_anyof_on_the_golden_sample(golden):  # noqa: F811
    shim, cwd = golden
    assert shim.n == 4
    for members in ([0], [1, 2], [3, 0]):
        _check(_anyof(shim, members, 4), _merged(shim, members, 4))
    t = shim.track_ids
    p = _run(["--playlist", f"{t[1]},{t[2]}", "--match", "any", "-n", "2"], cwd)
    assert p.returncode == 0, p.stdout + p.stderr
    ids, _, matched = _merged(shim, [1, 2], 2)
    assert _ids(p.stdout) == [t[i] for i in ids] and _matches(p.stdout) == [_name(shim, m) for m in matched]
    assert "Matching: the best of the playlist's songs (--match any)" in p.stdout and "=== PLAYLIST MODE ===" in p.stdout


def test_recommender_anyof(catalogue):  # noqa: F811
    shim, _ = catalogue
    members = [5, 70, 333, 5]                                     # a duplicate: the first occurrence is named
    for topn in (1, 10, 100):
        _check(_anyof(shim, members, topn), _merged(shim, members, topn))
        _check(_anyof(shim, members, topn, exclude=[1, 2, 3], where=(1, 0.2, 0.9)), _merged(shim, members, topn, [1, 2, 3], (1, 0.2, 0.9)))
    seen = list(range(0, shim.n, 3))
    assert shim.set_rows(seen) == 1                               # the row set of setRowSet applies
    _check(_anyof(shim, members, 20), _merged(shim, members, 20))
    shim.clear()
    for bit in (1, 2, 4, 8, 16, 32, 64):                          # refused with a message and {}
        assert _anyof(shim, members, 10, refuse=bit)[0] == []
    fn = shim.L.shim_set_candidates
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    a = np.asarray([1, 2, 3], np.int64)
    assert fn(shim.h, a.ctypes.data, 3) == 1
    assert _anyof(shim, members, 10)[0] == []                     # a set candidate list: refused
    assert fn(shim.h, None, -1) == 1
    assert shim.playlist([5], 3)[0] and _anyof(shim, [5], 3)[2] == [5, 5, 5]


def test_cli_match_any(catalogue):  # noqa: F811
    shim, cwd = catalogue
    t, n = shim.track_ids, shim.n
    members = [5, 70, 333]
    lk = ",".join(t[i] for i in members)
    seen = [int(i) for i in np.random.default_rng(5).permutation(n)[:200]]
    (cwd / "seen.txt").write_text("\n".join(t[i] for i in seen) + "\n")
    (cwd / "only.txt").write_text("\n".join(t[i] for i in seen) + "\n")
    (cwd / "list.txt").write_text(t[1] + "\n")
    (cwd / "priors.txt").write_text("0.5\n" * n)

    def transcript(more, want):
        p = _run(["--playlist", lk, "--match", "any", "-n", "8", *more], cwd)
        assert p.returncode == 0, (more, p.stdout, p.stderr)
        assert _ids(p.stdout) == [t[i] for i in want[0]], (more, p.stdout)
        assert _matches(p.stdout) == [_name(shim, m) for m in want[2]], (more, p.stdout)
        return p

    transcript([], _merged(shim, members, 8))
    transcript(["--where", "energy=0.2:0.9"], _merged(shim, members, 8, where=(1, 0.2, 0.9)))
    transcript(["--seen", "seen.txt"], _merged(shim, members, 8, exclude=seen))
    transcript(["--only", "only.txt"], _merged(shim, members, 8, exclude=[i for i in range(n) if i not in seen]))
    transcript(["--metric", "cosine"], _merged(shim, members, 8))
    p = _run(["--playlist", lk, "--match", "any", "-n", "8", "--genre", "rock", "--seen", "seen.txt"], cwd)
    assert p.returncode == 0 and len(_matches(p.stdout)) == len(_ids(p.stdout)) > 0 and not set(_ids(p.stdout)) & {t[i] for i in seen}
    assert all("Genre:  rock\n" in block for block in p.stdout.split("Recommendations:", 1)[1].split("\n\n") if "ID:" in block)
    # --match mean is no option at all
    a, b = _run(["--playlist", lk, "--match", "mean", "-n", "8"], cwd), _run(["--playlist", lk, "-n", "8"], cwd)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stderr == b.stderr and not _matches(a.stdout)
    # what does not combine, each with its message
    for more in REFUSED:
        p = _run(["--playlist", lk, "--match", "any", *[t[9] if x == "X" else x for x in more]], cwd)
        assert p.returncode == 1 and f"--match any cannot be combined with {more[0]} " in p.stderr, (more, p.stdout, p.stderr)
    p = _run(["--playlist", lk, "--match", "any", "--metric", "euclidean"], cwd)
    assert p.returncode == 1 and "--match any cannot be combined with --metric euclidean" in p.stderr
    for args, msg in ((["--playlist", lk, "--match"], "--match needs a name (mean or any)"),
                      (["--playlist", lk, "--match", "best"], "--match 'best': mean or any"),
                      (["--id", t[7], "--match", "any"], "--match goes with --playlist"),
                      (["--song", "Song 0007", "--match", "mean"], "--match goes with --playlist")):
        p = _run(args, cwd)
        assert p.returncode == 1 and msg in p.stderr, (args, p.stdout, p.stderr)
