"""Records tests/golden/cli_transcripts.json.gz (JSON, gzip): what the drop-in CLI (csrc/main.cpp) prints for a list of command lines.

RUN ON THE PARENT COMMIT, never on the code under test: check out the commit whose CLI is to be preserved, build it
(python __graft_entry__.py), copy THIS script and tests/cli_transcripts.py next to it if it lacks them, and run
    python tests/golden/make_cli_transcripts.py
from the repository root.  The CLI runs on the CPU backend (no HIP device visible), where two runs give identical bytes; the
scores and ids it prints are covered by the bit-exact contract between the CPU backend and the GPU.  tests/test_cli_transcripts.py
replays every case against the CLI of the tree under test.

A case is {"world", "argv", "exit", "stdout", "stderr"} (worlds: tests/cli_transcripts.py) and, for the twelve that the GPU test
replays, "gpu": true.
"""
from __future__ import annotations

import gzip
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import cli_transcripts as T  # noqa: E402

L = T.PLAYLIST
MODES = {"song": ["--song", "Song 0007"], "id": ["--id", "t0007"], "playlist": ["--playlist", L]}

# option -> argv; the second element: the modes that serve it
OPTIONS = {
    "genre": (["--genre", "rock"], "song id playlist"),
    "where": (["--where", "energy=0.2:0.9"], "song id playlist"),
    "diverse": (["--diverse", "0.5"], "song id playlist"),
    "cap": (["--max-per-artist", "1"], "song id playlist"),
    "euclid": (["--metric", "euclidean"], "song id playlist"),
    "scale": (["--scale", "key=0", "--scale", "tempo=2"], "song id playlist"),
    "seen": (["--seen", "seen.txt"], "song id playlist"),
    "only": (["--only", "only.txt"], "song id playlist"),
    "dislike": (["--dislike", "t0009"], "playlist"),
    "weights": (["--weights", "1,0.5,2"], "playlist"),
    "priors": (["--priors", "priors.txt", "--prior-weight", "0.5"], "playlist"),
}
REQUEST_ONLY = {"diverse", "cap", "dislike", "weights", "priors"}   # what --metric euclidean and --scale refuse


def combinable(mode, a, b):
    """Does the usage text call a and b combinable under `mode`?"""
    pair = {a, b}
    if pair == {"seen", "only"}:
        return False
    if pair & {"euclid", "scale"}:
        return not pair & REQUEST_ONLY
    if mode != "playlist" and "genre" in pair:
        return False
    return True


def cases():
    out = []

    def add(world, *argv, gpu=False):
        out.append({"world": world, "argv": list(argv), **({"gpu": True} if gpu else {})})

    names = list(OPTIONS)
    add("c600", "--preprocess", "songs.csv")
    for mode, head in MODES.items():
        add("c600", *head, "-n", "3", gpu=mode != "song")
        for name in names:                                           # every option alone
            argv, modes = OPTIONS[name]
            if mode in modes or (mode, name) == ("id", "weights"):   # (--id with a --playlist option: not looked at)
                shape = mode == "playlist" and name != "only" or (mode, name) == ("id", "genre")
                gpu = shape and name != "dislike"
                add("c600", *head, *argv, "-n", "3" if gpu else "2", gpu=gpu)
        for i, a in enumerate(names):                                # every pair: served, or refused
            for b in names[i + 1:]:
                if mode not in OPTIONS[a][1] or mode not in OPTIONS[b][1] or mode == "song" and combinable(mode, a, b):
                    continue                                         # (--song: the refusals only; --id runs the same code for the rest)
                add("c600", *head, *OPTIONS[a][0], *OPTIONS[b][0], "-n", "1")
    P, I, S = MODES["playlist"], MODES["id"], MODES["song"]
    add("c600", *P, "--dislike", "t0009", "--dislike-weight", "0.25", "--weights", "2,1,1", "-n", "2")
    add("c600", *P, "--diverse", "0.5", "--pool", "40", "-n", "2")
    add("c600", *I, "--diverse", "0.5", "--pool", "40", "-n", "2")
    add("c600", *P, "--max-per-artist", "2", "--pool", "40", "-n", "3")
    add("c600", *P, "--max-per-artist", "1", "--diverse", "0.3", "--genre", "rock", "--genre", "JAZZ", "-n", "3")
    add("c600", *P, "--diverse", "1", "--genre", "rock", "-n", "3")                 # the plain-request shortcut
    add("c600", *P, "--priors", "priors.txt", "--prior-weight", "0", "-n", "3")
    add("c600", *P, "--priors", "priors.txt", "--prior-weight", "-2", "--genre", "pop", "--max-per-artist", "1", "-n", "3")
    add("c600", *P, "--metric", "cosine", "--diverse", "0.5", "-n", "2")
    add("c600", *P, "--metric", "euclidean", "--metric", "cosine", "-n", "2")
    add("c600", *S, "--metric", "euclidean", "--scale", "mode=0", "--genre", "pop", "--where", "valence=0:0.5", "-n", "2")
    add("c600", *I, "--scale", "genre=0", "--seen", "seen.txt", "--genre", "metal", "-n", "2")
    add("c600", *P, "--where", "energy=0.2:0.9", "--where", "energy=0.5:1", "--where", "tempo=0:0.8", "-n", "2")
    add("c600", "--playlist", "t0007", "--genre", "rock", "--seen", "seen.txt", "--where", "key=0:0.5", "-n", "2")
    add("c600", "--song", "song 059", "-n", "2")                                      # a substring
    add("c600", "--song", "song 059", "--diverse", "0.5", "-n", "2")
    # the refusals beyond the pairs above
    for head in (I, P):
        add("c600", *head, "--pool", "40", "-n", "2")
        add("c600", *head, "--diverse", "0.5", "--pool", "2", "-n", "3")
        add("c600", *head, "--seen", "seen.txt", "--seen", "seen.txt")
        for opt in ("--pool", "--dislike-weight", "--prior-weight"):
            add("c600", *head, "--metric", "euclidean", opt, "1")
            add("c600", *head, opt, "1", "--scale", "key=0")
        add("c600", *head, "--pool", "5", "--diverse", "0.5", "--metric", "euclidean")   # (the first in argv is named)
    add("c600", *I, "--max-per-artist", "2", "--diverse", "0.5", "--genre", "rock")
    add("c600", *P, "--priors", "priors.txt")
    add("c600", *P, "--prior-weight", "1")
    # malformed values
    bad = [["--where"], ["--where", "energy"], ["--where", "energy=0.5"], ["--where", "bogus=0:1"], ["--where", "energy=a:b"],
           ["--where", "energy=:1"], ["--where", "energy=0.9:0.2"], ["--scale"], ["--scale", "key"], ["--scale", "bogus=1"],
           ["--scale", "key=x"], ["--scale", "key=-1"], ["--scale", "key=2000"], ["--scale", "key=0", "--metric"],
           ["--metric"], ["--metric", "manhattan"], ["--diverse"], ["--diverse", "x"], ["--diverse", "1.5"], ["--pool"],
           ["--diverse", "0.5", "--pool", "0"], ["--diverse", "0.5", "--pool", "x"], ["--max-per-artist"], ["--max-per-artist", "0"],
           ["--max-per-artist", "x"], ["--seen"], ["--only"], ["--seen", "missing.txt"], ["--only", "missing.txt"], ["--genre"],
           ["--genre", "nosuchgenre"], ["-n", "0"], ["-n", "abc"], ["-n", "-4"]]
    for b in bad:
        add("c600", *P, *b)
    for b in bad[::2]:                                               # (the same parsers: every other one under --id too)
        add("c600", *I, *b)
    for b in (["--dislike"], ["--dislike-weight"], ["--dislike-weight", "x"], ["--dislike-weight", "-1"], ["--weights"], ["--weights", "1,x,2"],
              ["--weights", "1,2"], ["--weights", "0,0,0"], ["--dislike", "nosuchid"], ["--priors"], ["--prior-weight"],
              ["--priors", "priors.txt", "--prior-weight", "9"], ["--priors", "priors.txt", "--prior-weight", "x"],
              ["--priors", "missing.txt", "--prior-weight", "1"], ["--priors", "priors_short.txt", "--prior-weight", "1"],
              ["--priors", "priors_text.txt", "--prior-weight", "1"], ["--priors", "priors_range.txt", "--prior-weight", "1"]):
        add("c600", *P, *b)
    add("c600", *S, "--genre", "nosuchgenre")
    add("c600", *S, "--where", "bogus=0:1")
    add("c600", *S, "-n", "0")
    # two malformed options in one command line, in both orders
    twos = [(["--where", "bogus=0:1"], ["--scale", "bogus=1"]), (["--diverse", "x"], ["--weights", "x"]), (["--metric", "manhattan"], ["--where", "energy"]),
            (["--prior-weight", "x"], ["--diverse", "0.5", "--pool", "0"]), (["--seen"], ["--genre"]), (["-n", "0"], ["--where", "energy"]),
            (["--max-per-artist", "x"], ["--dislike-weight", "-1"]), (["--scale", "key=x"], ["--only", "only.txt", "--seen", "seen.txt"])]
    for a, b in twos:
        for head in (I, P):
            add("c600", *head, *a, *b)
            if a[-1] not in ("--seen",) and b[-1] not in ("--genre",):   # (an option without its value has to stand last)
                add("c600", *head, *b, *a)
    # a refusal and a malformed value in one command line, in both orders: the one reported is the one whose option is parsed first
    # (--metric's refusals before --scale is parsed, --genre beside --diverse or a cap after their values are)
    mixed = [(["--metric", "euclidean", "--diverse", "0.5"], ["--scale", "bogus=1"]), (["--metric", "euclidean"], ["--diverse", "x"]),
             (["--scale", "key=0"], ["--diverse", "x"]), (["--scale", "key=0"], ["--max-per-artist", "0"]),
             (["--metric", "euclidean"], ["--pool", "x"]), (["--metric", "manhattan"], ["--scale", "key=0", "--pool", "5"])]
    for a, b in mixed:
        for head in (I, P):
            add("c600", *head, *a, *b)
            add("c600", *head, *b, *a)
    add("c600", *I, "--metric", "euclidean", "--pool", "5", "--scale")
    for a, b in ((["--metric", "euclidean"], ["--weights", "x"]), (["--scale", "key=0"], ["--prior-weight", "x"]),
                 (["--seen", "seen.txt", "--only", "only.txt"], ["--metric", "manhattan"]), (["--seen", "seen.txt", "--only", "only.txt"], ["--where", "energy"])):
        add("c600", *P, *a, *b)
        add("c600", *P, *b, *a)
    for a, b in ((["--genre", "rock"], ["--diverse", "x"]), (["--genre", "rock"], ["--max-per-artist", "2", "--pool", "1", "-n", "3"]),
                 (["--genre", "rock", "--where", "energy=0.2:0.9"], ["--diverse", "x"]), (["--genre", "rock", "--seen", "seen.txt"], ["--max-per-artist", "0"]),
                 (["--genre", "rock"], ["--where", "bogus=0:1"]), (["--genre", "rock", "--where", "energy=0.2:0.9"], ["--metric", "manhattan"]),
                 (["--genre", "rock", "--seen", "seen.txt"], ["--scale", "key=x"]), (["--genre", "rock", "--diverse", "0.5"], ["--scale", "key=x"]),
                 (["--pool", "40"], ["--max-per-artist", "x"]), (["--genre", "rock", "--pool", "40"], ["-n", "0"])):
        add("c600", *I, *a, *b)
        add("c600", *I, *b, *a)
    add("c600", *S, "--genre", "rock", "--diverse", "x")
    add("c600", *S, "--diverse", "0.5", "--genre", "rock", "--scale", "key=x")
    add("c600", *I, "--pool", "x")
    add("c600", *P, "--genre", "--seen")
    add("c600", *I, "--genre", "--seen")
    # -n: the first among argv[3 .. argc-2] counts; in last position it is not looked at
    add("c600", *I, "-n")
    add("c600", "--playlist", "t0005", "--where", "energy=0.2:0.9", "-n")
    add("c600", *I, "-n", "2", "-n", "4")
    add("c600", *P, "--genre", "rock", "-n", "2")
    add("c600", *S, "-n", "2", "--genre", "rock")
    add("sample", "--id", "dupA", "-n", "2000000000")
    # what is not there
    add("c600", "--song", "no such song", "-n", "2")
    add("c600", "--id", "nosuchid", "-n", "2")
    for more in (["--where", "energy=0.2:0.9"], ["--diverse", "0.5"], ["--max-per-artist", "1"], ["--genre", "rock"], ["--metric", "euclidean"],
                 ["--seen", "seen.txt"]):
        add("c600", "--id", "nosuchid", *more)
        add("c600", "--song", "no such song", *more)
    add("c600", "--playlist", "t0001,nosuchid", "-n", "2")
    add("c600", "--playlist", "t0001,nosuchid", "--metric", "euclidean")
    add("c600", "--playlist", ",", "-n", "2")
    add("c600", "--playlist", ",", "--scale", "key=0")
    add("c600", "--playlist", ",".join(f"t{i:04d}" for i in range(33)), "-n", "2")
    add("c600", *P, "--genre", "nosuchgenre", "--metric", "euclidean")
    add("c600", *I, "--seen", "seen_unknown.txt", "-n", "2")
    add("c600", *P, "--only", "seen_unknown.txt", "-n", "2")
    add("c600", *P, "--only", "priors_short.txt", "-n", "2")                          # a set that names no song: nothing to rank
    add("empty", "--id", "t0007")
    add("empty", *P, "--genre", "rock")
    add("empty", *P, "--metric", "euclidean")
    add("empty", "--preprocess", "missing.csv")
    add("empty")
    add("empty", "--bogus")
    add("empty", "--preprocess")
    add("empty", "--song")
    add("empty", "--playlist")
    # the four-song sample and the name rules
    add("sample", "--song", "lala")
    add("sample", "--song", "Gen Z", "--genre", "dance", "-n", "2")
    add("sample", "--id", "dupA", "-n", "2")
    add("sample", "--id", "dupA", "--diverse", "0.5", "-n", "10")
    add("sample", "--id", "dupA", "--max-per-artist", "1", "-n", "10")
    add("sample", "--id", "dupA", "--where", "energy=0:1", "-n", "10")
    add("sample", "--id", "dupA", "--metric", "euclidean", "-n", "10")
    add("sample", "--playlist", "dupA,5SuOikwiRyPMVoIQDJUgSV", "-n", "4")
    add("sample", "--playlist", "dupA", "--seen", "sample_seen.txt", "-n", "4")
    add("sample", "--id", "5SuOikwiRyPMVoIQDJUgSV", "--only", "sample_seen.txt", "-n", "4")
    for more in ([], ["--where", "energy=0:1"], ["--diverse", "0.5"], ["--genre", "rock"], ["--metric", "euclidean"], ["--scale", "key=0"]):
        add("names", "--song", "alpha", *more, "-n", "2")
    return out


def main():
    from spotify_recommender_amd import build
    env = T.environment()
    recorded = []
    with tempfile.TemporaryDirectory() as tmp:
        worlds = T.make_worlds(tmp, build.BIN_CLI, env)
        for case in cases():
            cwd = worlds[case["world"]]
            if case["argv"][:1] == ["--preprocess"] and (cwd / "songs_data.bin").exists():
                (cwd / "songs_data.bin").unlink()                    # (written again by the case)
            a, b = (T.run(build.BIN_CLI, case["argv"], cwd, env) for _ in range(2))
            assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr), case["argv"]
            recorded.append({**case, "exit": a.returncode, "stdout": a.stdout, "stderr": a.stderr})
    text = T.dump_cases(recorded)
    T.FIXTURE.write_bytes(gzip.compress(text, 9, mtime=0))   # (mtime 0: the same bytes for the same transcripts)
    gpu = sum(1 for c in recorded if c.get("gpu"))
    print(f"{len(recorded)} cases ({gpu} for the GPU test), {sum(c['exit'] != 0 for c in recorded)} with a non-zero exit, "
          f"{len(text)} bytes of JSON, {T.FIXTURE.stat().st_size} packed")


if __name__ == "__main__":
    main()
