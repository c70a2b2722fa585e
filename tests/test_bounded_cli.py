"""BOUNDED REQUESTS through the C++ drop-in and the CLI (include/Recommender.h: Query::atLeast, Query::within, lastMatchCount;
csrc/main.cpp: --min-score S, --within R with --metric euclidean, --count-only), on a 600-song catalogue against
tests/bounded_oracle.py: the recommendations, their values, the "N of TOTAL matching" line, beside --where, --seen, --only and
--genre; every refusal with its message; a command line without the new options prints what it printed before."""
import ctypes
import re

import numpy as np
import pytest

from tests import bounded_oracle as bo
from tests.test_rowset_cli import Shim, _ids, _run, catalogue  # noqa: F401  (catalogue: the fixture)

REFUSED = (["--weights", "1,1,1"], ["--dislike", "X"], ["--dislike-weight", "0.5"], ["--diverse", "0.5"], ["--pool", "50"],
           ["--max-per-artist", "1"], ["--priors", "priors.txt"], ["--prior-weight", "0.5"], ["--scale", "key=0"],
           ["--candidates", "list.txt"], ["--score", "list.txt"])


def _features(shim):
    fn = shim.L.shim_song_features
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    out = np.zeros((shim.n, 12), np.float32)
    genre = ctypes.c_int(0)
    for i in range(shim.n):
        assert fn(shim.h, i, out[i].ctypes.data, ctypes.byref(genre)) == 1
    return out


def _bounded(shim, songs, topn, bound, euclidean=False, exclude=(), where=None, refuse=0):
    fn = shim.L.shim_query_bounded
    fn.restype = ctypes.c_int64
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fn.argtypes = [P, P, I, P, I, I, F, F, I, I, F, I, P, P, P, ctypes.c_int64]
    s, ex = np.asarray(songs, np.int32), np.asarray(list(exclude) or [0], np.int32)
    out, sc = np.full(1024, -7, np.int32), np.zeros(1024, np.float32)
    total = ctypes.c_longlong(-9)
    f, lo, hi = where if where is not None else (-1, 0.0, 0.0)
    n = fn(shim.h, s.ctypes.data, len(songs), ex.ctypes.data, len(exclude), f, lo, hi, topn, int(euclidean), bound, refuse, out.ctypes.data,
           sc.ctypes.data, ctypes.byref(total), 1024)
    assert n >= 0
    return out[:n].astype(np.int64), sc[:n].copy(), int(total.value)


def _values(stdout, word):
    return re.findall(r'^\d+\. ".*"  \(' + word + r' (.*)\)$', stdout.split("Recommendations:", 1)[1], flags=re.M)


def _matching(stdout):
    m = re.search(r"^(\d+) of (\d+) matching \((score >=|distance <=) (\S+)\)$", stdout, flags=re.M)
    assert m, stdout
    return int(m.group(1)), int(m.group(2))


def test_recommender_at_least_and_within(catalogue):  # noqa: F811
    shim, _ = catalogue
    feats = _features(shim)
    members = [5, 70, 333]
    for metric, euclid in ((bo.COSINE, False), (bo.EUCLIDEAN, True)):
        v = bo.values(feats, feats[members], metric)
        ok = bo.admissible(feats, v, members)
        ok_x = bo.admissible(feats, v, members + [1, 2, 3], {1: (0.2, 0.9)})
        for bound in bo.bounds_for(v, ok, metric):
            total = bo.expected_from_values(v, ok, metric, bound, 0)[2]
            for topn in sorted({0, 1, 10, min(shim.n, total + 1)}):
                bo.check(_bounded(shim, members, topn, bound, euclid), bo.expected_from_values(v, ok, metric, bound, topn), f"{metric} {bound!r} top-{topn}")
            bo.check(_bounded(shim, members, 10, bound, euclid, exclude=[1, 2, 3], where=(1, 0.2, 0.9)),
                     bo.expected_from_values(v, ok_x, metric, bound, 10), f"{metric} {bound!r}, exclusion and range")
        seen = list(range(0, shim.n, 3))
        assert shim.set_rows(seen) == 1                           # the row set of setRowSet applies
        bound = bo.bounds_for(v, ok, metric)[-2]
        bo.check(_bounded(shim, members, 20, bound, euclid),
                 bo.expected_from_values(v, bo.admissible(feats, v, members, rowset=seen), metric, bound, 20), "row set")
        shim.clear()
        for bit in (1, 2, 4, 8, 16, 64, 128, 256, 512):           # refused with a message and {}; no count is left behind
            got = _bounded(shim, members, 10, bound, euclid, refuse=bit)
            assert got[0].size == 0 and (bit == 64 or got[2] == -1), (bit, got)
        bo.check(_bounded(shim, members, 10, bound, euclid), bo.expected_from_values(v, ok, metric, bound, 10), "after the refusals")
    assert shim.playlist(members, 5)[0] and _bounded(shim, members, 5, 0.0)[2] >= 0


def test_cli_min_score_within_and_count_only(catalogue):  # noqa: F811
    shim, cwd = catalogue
    feats = _features(shim)
    t, n = shim.track_ids, shim.n
    members = [5, 70, 333]
    lk = ",".join(t[i] for i in members)
    seen = [int(i) for i in np.random.default_rng(5).permutation(n)[:200]]
    (cwd / "seen.txt").write_text("\n".join(t[i] for i in seen) + "\n")
    (cwd / "list.txt").write_text(t[1] + "\n")
    (cwd / "priors.txt").write_text("0.5\n" * n)

    def transcript(args, metric, bound, want, topn=8):
        opts = ["--min-score", repr(bound)] if metric == bo.COSINE else ["--metric", "euclidean", "--within", repr(bound)]
        p = _run([*args, *opts, "-n", str(topn)], cwd)
        assert p.returncode == 0, (args, p.stdout, p.stderr)
        assert ("=== BOUNDED MODE (similarity at least a score) ===" if metric == bo.COSINE else "=== BOUNDED MODE (within a Euclidean distance) ===") in p.stdout
        assert _matching(p.stdout) == (want[0].size, want[2]), (args, p.stdout)
        if want[0].size:
            assert _ids(p.stdout) == [t[i] for i in want[0]], (args, p.stdout)
            got = _values(p.stdout, "score" if metric == bo.COSINE else "distance")
            assert [np.float32(x) for x in got] == pytest.approx(want[1].tolist(), rel=1e-5), (args, p.stdout)
        else:
            assert "Recommendations:" not in p.stdout and "Recommendation complete!" in p.stdout
        return p

    for metric in (bo.COSINE, bo.EUCLIDEAN):
        v = bo.values(feats, feats[members], metric)
        ok = bo.admissible(feats, v, members)
        bounds = bo.bounds_for(v, ok, metric)
        # (the CLI parses the bound as fp32 from its shortest decimal form: repr of a float that is an fp32 value round-trips)
        for bound in (bounds[-2], bounds[-1], bounds[4] if metric == bo.COSINE else bounds[2], bounds[1]):
            transcript(["--playlist", lk], metric, bound, bo.expected_from_values(v, ok, metric, bound, 8))
        bound = bounds[-2]
        transcript(["--playlist", lk, "--where", "energy=0.2:0.9"], metric, bound,
                   bo.expected_from_values(v, bo.admissible(feats, v, members, {1: (0.2, 0.9)}), metric, bound, 8))
        transcript(["--playlist", lk, "--seen", "seen.txt"], metric, bound,
                   bo.expected_from_values(v, bo.admissible(feats, v, members, rowset=seen), metric, bound, 8))
        transcript(["--playlist", lk, "--only", "seen.txt"], metric, bound,
                   bo.expected_from_values(v, bo.admissible(feats, v, members, rowset=seen, rowset_only=True), metric, bound, 8))
        one = bo.values(feats, feats[[7]], metric)
        ok1 = bo.admissible(feats, one, [7])
        b1 = bo.bounds_for(one, ok1, metric)[-2]
        transcript(["--id", t[7]], metric, b1, bo.expected_from_values(one, ok1, metric, b1, 8))
        transcript(["--song", "Song 0007"], metric, b1, bo.expected_from_values(one, ok1, metric, b1, 8))
        # --count-only: the number alone, whatever -n says
        opts = ["--min-score", repr(bound)] if metric == bo.COSINE else ["--metric", "euclidean", "--within", repr(bound)]
        p = _run(["--playlist", lk, *opts, "--count-only", "-n", "8"], cwd)
        assert p.returncode == 0 and _matching(p.stdout) == (0, bo.expected_from_values(v, ok, metric, bound, 0)[2]), (p.stdout, p.stderr)
        assert "Recommendations:" not in p.stdout
        p = _run(["--playlist", lk, *opts, "-n", "8", "--genre", "rock", "--seen", "seen.txt"], cwd)
        assert p.returncode == 0 and not set(_ids(p.stdout)) & {t[i] for i in seen} and _matching(p.stdout)[0] == len(_ids(p.stdout)) > 0
        assert all("Genre:  rock\n" in block for block in p.stdout.split("Recommendations:", 1)[1].split("\n\n") if "ID:" in block)
    # what does not combine, each with its message
    for more in REFUSED:
        p = _run(["--playlist", lk, "--min-score", "0.9", *[t[9] if x == "X" else x for x in more]], cwd)
        assert p.returncode == 1 and f"a bound (--min-score, --within) cannot be combined with {more[0]} " in p.stderr, (more, p.stdout, p.stderr)
    for args, msg in ((["--min-score", "0.9", "--match", "any"], "a bound (--min-score, --within) cannot be combined with --match any"),
                      (["--min-score", "0.9", "--distance", "manhattan"], "a bound (--min-score, --within) cannot be combined with --distance manhattan"),
                      (["--min-score"], "--min-score needs a number"), (["--min-score", "high"], "--min-score 'high': a finite number"),
                      (["--min-score", "nan"], "--min-score 'nan': a finite number"), (["--min-score", "inf"], "--min-score 'inf': a finite number"),
                      (["--min-score", "0.9", "--min-score", "0.8"], "--min-score cannot be combined with --min-score (one bound per request)"),
                      (["--within", "0.5"], "--within goes with --metric euclidean (a score floor is --min-score S)"),
                      (["--metric", "euclidean", "--min-score", "0.5"], "--min-score cannot be combined with --metric euclidean (a radius is --within R)"),
                      (["--metric", "euclidean", "--within", "-1"], "--within '-1': a radius is >= 0"),
                      (["--count-only"], "--count-only goes with --min-score or --within")):
        p = _run(["--playlist", lk, *args], cwd)
        assert p.returncode == 1 and "Error: " + msg in p.stderr, (args, p.stdout, p.stderr)
