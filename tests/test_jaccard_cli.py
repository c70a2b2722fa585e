"""JACCARD REQUESTS through the CLI (csrc/main.cpp: --similarity jaccard), every child with no device visible (the CPU backend): on
tests/golden/sample_songs.csv the banner, the "(similarity S)" tail of every recommendation, --song / --id / --playlist, and the
refusal beside every option it does not go with; on a 600-song catalogue the recommendations and their values against
tests/jaccard_oracle.py beside --where, --seen, --only and --genre.  A command line without the option prints what it printed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.jaccard_oracle import expected_from_v, mean_jaccard
from tests.test_jaccard_cpu import features_of
from tests.test_rowset_cli import Shim, _ids, catalogue  # noqa: F401  (catalogue: the fixture)

BANNER = "=== RECOMMENDATION MODE (Jaccard similarity) ==="
ONLY = "(Jaccard requests take --genre, --where, --seen and --only only)"
REFUSED = (["--weights", "1,1,1"], ["--dislike", "X"], ["--dislike-weight", "0.5"], ["--diverse", "0.5"], ["--pool", "50"],
           ["--max-per-artist", "1"], ["--priors", "priors.txt"], ["--prior-weight", "0.5"], ["--scale", "key=0"],
           ["--candidates", "list.txt"], ["--score", "list.txt"], ["--metric", "euclidean"], ["--metric", "cosine"],
           ["--distance", "manhattan"], ["--match", "any"], ["--min-score", "0.5"], ["--within", "0.5"], ["--count-only"])


def _run(args, cwd):
    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def _entries(stdout):
    """Every numbered line under "Recommendations:" as (whole line, similarity text or None)."""
    lines = [l for l in stdout.split("Recommendations:", 1)[1].splitlines() if re.match(r'^\d+\. "', l)]
    return [(l, (re.search(r'"  \(similarity (\S+)\)$', l) or [None, None])[1]) for l in lines]


def test_cli_on_the_golden_sample(engine_lib, golden_dir, tmp_path):
    from spotify_recommender_amd import build
    build.build_shim()
    shutil.copy(golden_dir / "sample_songs.csv", tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    seed = "5SuOikwiRyPMVoIQDJUgSV"
    p = _run(["--id", seed, "-n", "1000", "--similarity", "jaccard"], tmp_path)
    assert p.returncode == 0 and BANNER in p.stdout and "Recommendation complete!" in p.stdout, p.stdout + p.stderr
    ids, entries = _ids(p.stdout), _entries(p.stdout)
    assert len(ids) == len(entries) == 3 and seed not in ids
    sims = [float(s) for _, s in entries]                         # (every line ends in its similarity)
    assert sims == sorted(sims, reverse=True) and all(0.0 <= s <= 1.0 for s in sims)
    # the same song as a one-song playlist and by name
    for args in (["--playlist", seed], ["--song", "Gen Z"]):
        q = _run([*args, "-n", "1000", "--similarity", "jaccard"], tmp_path)
        assert q.returncode == 0 and BANNER in q.stdout and (_ids(q.stdout), _entries(q.stdout)) == (ids, entries), q.stdout + q.stderr
    # with --genre and --where
    g = _run(["--playlist", seed, "-n", "3", "--similarity", "jaccard", "--genre", "rock", "--genre", "dance", "--where", "energy=0:1"], tmp_path)
    assert g.returncode == 0 and "Restricted to genres: rock dance" in g.stdout and BANNER in g.stdout, g.stdout + g.stderr
    assert _ids(g.stdout) and set(_ids(g.stdout)) <= set(ids) and all(s is not None for _, s in _entries(g.stdout))
    # what does not combine, each with its message and exit 1
    (tmp_path / "list.txt").write_text(ids[0] + "\n")
    (tmp_path / "priors.txt").write_text("0.5\n" * 4)
    for more in REFUSED:
        r = _run(["--playlist", seed, "--similarity", "jaccard", *["dupA" if x == "X" else x for x in more]], tmp_path)
        assert r.returncode == 1 and f"Error: --similarity jaccard cannot be combined with {more[0]} {ONLY}" in r.stderr, (more, r.stdout, r.stderr)
        assert "Recommendations:" not in r.stdout
    for args, msg in ((["--similarity"], "--similarity needs a name (jaccard)"), (["--similarity", "dice"], "--similarity 'dice': jaccard")):
        r = _run(["--id", seed, *args], tmp_path)
        assert r.returncode == 1 and "Error: " + msg in r.stderr, (args, r.stdout, r.stderr)
    # --metric and --distance keep their names, and a plain run neither the banner nor the tails
    assert "cosine or euclidean" in _run(["--id", seed, "--metric", "jaccard"], tmp_path).stderr
    assert "--distance 'jaccard': manhattan" in _run(["--id", seed, "--distance", "jaccard"], tmp_path).stderr
    c = _run(["--id", seed, "-n", "3"], tmp_path)
    assert c.returncode == 0 and "Jaccard" not in c.stdout and "(similarity" not in c.stdout and "=== RECOMMENDATION MODE ===" in c.stdout


def test_cli_against_the_oracle(catalogue):  # noqa: F811
    shim, cwd = catalogue
    feats = features_of(shim)
    t, n = shim.track_ids, shim.n
    members = [5, 70, 333]
    vv = mean_jaccard(feats, feats[members])
    lk = ",".join(t[i] for i in members)
    seen = [int(i) for i in np.random.default_rng(5).permutation(n)[:200]]
    (cwd / "seen.txt").write_text("\n".join(t[i] for i in seen) + "\n")

    def transcript(args, want):
        p = _run([*args, "--similarity", "jaccard", "-n", "8"], cwd)
        assert p.returncode == 0 and BANNER in p.stdout, (args, p.stdout, p.stderr)
        assert _ids(p.stdout) == [t[i] for i in want[0]], (args, p.stdout)
        assert [np.float32(s) for _, s in _entries(p.stdout)] == pytest.approx(want[1].tolist(), rel=1e-5), (args, p.stdout)
        return p

    transcript(["--playlist", lk], expected_from_v(feats, vv, members, 8))
    transcript(["--playlist", lk, "--where", "energy=0.2:0.9"], expected_from_v(feats, vv, members, 8, {1: (0.2, 0.9)}))
    transcript(["--playlist", lk, "--seen", "seen.txt"], expected_from_v(feats, vv, members, 8, rowset=seen))
    transcript(["--playlist", lk, "--only", "seen.txt"], expected_from_v(feats, vv, members, 8, rowset=seen, rowset_only=True))
    one = mean_jaccard(feats, feats[[7]])
    transcript(["--id", t[7]], expected_from_v(feats, one, [7], 8))
    transcript(["--song", "Song 0007"], expected_from_v(feats, one, [7], 8))
    p = _run(["--playlist", lk, "--similarity", "jaccard", "-n", "8", "--genre", "rock", "--seen", "seen.txt"], cwd)
    assert p.returncode == 0 and len(_entries(p.stdout)) == len(_ids(p.stdout)) > 0 and not set(_ids(p.stdout)) & {t[i] for i in seen}
    assert all("Genre:  rock\n" in block for block in p.stdout.split("Recommendations:", 1)[1].split("\n\n") if "ID:" in block)
