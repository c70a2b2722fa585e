"""CANDIDATE LISTS through the C++ drop-in and the CLI (include/Recommender.h: setCandidates / clearCandidates; csrc/main.cpp:
--candidates FILE), on a 600-song catalogue: a list against the ONLY row set of the same songs (setRowSet(..., true), --only FILE),
beside a listening history (--seen), --where, --metric euclidean, --scale, --diverse, --max-per-artist and --genre; unknown ids
(skipped, counted on stderr), an unreadable file and a repeated flag (exit 1)."""
import ctypes

import numpy as np

from tests.test_rowset_cli import Shim, _ids, _run, _same, catalogue  # noqa: F401  (catalogue: the fixture)


def _set_candidates(shim, rows):
    fn = shim.L.shim_set_candidates
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    if rows is None:
        return fn(shim.h, None, -1)
    a = np.asarray(list(rows) or [0], np.int64)
    return fn(shim.h, a.ctypes.data, len(rows))


def test_recommender_candidates(catalogue):  # noqa: F811
    shim, _ = catalogue
    n = shim.n
    rng = np.random.default_rng(3)
    cand = [int(i) for i in rng.permutation(n)[:250]]
    seen = [int(i) for i in rng.permutation(n)[:300]]
    members = [5, 70, 333]
    plain = shim.playlist(members, 50)
    assert shim.set_rows(cand, only=True) == 1
    want, want_w = shim.playlist(members, 50), shim.playlist(members, 50, where=(1, 0.2, 0.9))
    assert shim.set_rows([c for c in cand if c not in seen], only=True) == 1
    want_unseen = shim.playlist(members, 50)
    shim.clear()
    assert _set_candidates(shim, cand + cand[:5]) == 1                      # any order, duplicates allowed
    _same(shim.playlist(members, 50), want)
    _same(shim.playlist(members, 50, where=(1, 0.2, 0.9)), want_w)
    assert shim.set_rows(seen) == 1                                         # candidates minus a listening history
    _same(shim.playlist(members, 50), want_unseen)
    shim.clear()
    assert _set_candidates(shim, [1, n]) == 0 and _set_candidates(shim, [-1]) == 0    # refused: the list stays as it was
    _same(shim.playlist(members, 50), want)
    assert _set_candidates(shim, []) == 1                                   # an empty list is a list
    assert shim.playlist(members, 50)[0] == []
    assert _set_candidates(shim, None) == 1
    _same(shim.playlist(members, 50), plain)


def test_cli_candidates(catalogue):  # noqa: F811
    shim, cwd = catalogue
    t, n = shim.track_ids, shim.n
    rng = np.random.default_rng(5)
    cand = [int(i) for i in rng.permutation(n)[:220]]
    seen = [int(i) for i in rng.permutation(n)[:200]]
    (cwd / "cand.txt").write_text("\n".join([t[i] for i in cand] + ["unknown-a", "", t[cand[0]]]) + "\n")
    (cwd / "only.txt").write_text("\n".join(t[i] for i in cand) + "\n")
    (cwd / "seen.txt").write_text("\n".join(t[i] for i in seen) + "\n")
    (cwd / "unseen.txt").write_text("\n".join(t[i] for i in cand if i not in seen) + "\n")
    lk = ",".join(t[i] for i in (5, 70, 333))
    a = _run(["--playlist", lk, "--candidates", "cand.txt", "-n", "8"], cwd)
    b = _run(["--playlist", lk, "--only", "only.txt", "-n", "8"], cwd)
    assert a.returncode == 0 and b.returncode == 0, a.stdout + a.stderr + b.stderr
    assert _ids(a.stdout) == _ids(b.stdout) and len(_ids(a.stdout)) == 8 and set(_ids(a.stdout)) <= {t[i] for i in cand}
    assert "221 tracks, 1 lines skipped" in a.stderr and "Ranking 221 listed candidates" in a.stdout
    for mode, query in (("--id", t[7]), ("--song", "Song 0007")):
        a = _run([mode, query, "--candidates", "cand.txt", "-n", "6"], cwd)
        b = _run([mode, query, "--only", "only.txt", "-n", "6"], cwd)
        assert a.returncode == 0 and _ids(a.stdout) == _ids(b.stdout), a.stdout + a.stderr
    for more in ([], ["--where", "energy=0.2:0.9"], ["--metric", "euclidean"], ["--scale", "key=0", "--scale", "tempo=2"],
                 ["--diverse", "0.5"], ["--max-per-artist", "1"], ["--genre", "rock"], ["--dislike", t[9]]):
        a = _run(["--playlist", lk, "--candidates", "cand.txt", "--seen", "seen.txt", "-n", "8", *more], cwd)
        b = _run(["--playlist", lk, "--only", "unseen.txt", "-n", "8", *more], cwd)
        assert a.returncode == 0 and b.returncode == 0, (more, a.stderr, b.stderr)
        assert _ids(a.stdout) == _ids(b.stdout) and _ids(a.stdout), (more, a.stdout)
    for bad, msg in ((["--candidates", "missing.txt"], "cannot open the candidate list file 'missing.txt'"), (["--candidates"], "needs a file"),
                     (["--candidates", "cand.txt", "--candidates", "cand.txt"], "once")):
        p = _run(["--playlist", lk, *bad], cwd)
        assert p.returncode == 1 and msg in p.stderr, (bad, p.stdout, p.stderr)
    p = _run(["--id", t[7], "--candidates", "cand.txt", "--genre", "rock"], cwd)
    assert p.returncode == 1 and "--playlist <one id>" in p.stderr
