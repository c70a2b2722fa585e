"""What tests/golden/make_cli_transcripts.py (the recorder) and tests/test_cli_transcripts.py (the replay) share: the working
directories ("worlds") a command line of tests/golden/cli_transcripts.json.gz runs in, the side files they hold, how the CLI is
started, and the lines that a comparison leaves out."""
import os
import shutil
import subprocess
from pathlib import Path

GOLD = Path(__file__).resolve().parent / "golden"
FIXTURE = GOLD / "cli_transcripts.json.gz"   # (gzip: some three hundred transcripts are 247 kB of text, 11 kB packed)


def load_cases():
    import gzip
    import json
    return json.loads(gzip.decompress(FIXTURE.read_bytes()).decode())["cases"]


def dump_cases(cases) -> bytes:
    """The fixture's JSON (before gzip): one case per line."""
    import json
    lines = ",\n".join(json.dumps(c, separators=(",", ":"), ensure_ascii=False) for c in cases)
    return ('{"cases":[\n' + lines + "\n]}\n").encode()

# the 600-song catalogue (tests/test_playlist_cpu.py::_write_csv, seed 4): t0000..t0599, "Song 0000".., 37 artists, 5 genres
PLAYLIST = "t0005,t0070,t0333"

# "names": a song whose name CONTAINS the query stands before the song whose name IS the query (--song ranks by the second and
# displays the first)
NAMES_CSV = """\
track_id,track_name,artists,danceability,energy,key,loudness,mode,speechiness,acousticness,instrumentalness,liveness,valence,tempo,track_genre
n0,Alpha Beta,One,0.60,0.88,0,-3.8,1,0.18,0.03,0.0,0.08,0.36,133.0,dance
n1,Alpha,Two,0.74,0.69,8,-6.5,0,0.07,0.10,0.0,0.09,0.84,130.0,dance
n2,Gamma,Three,0.49,0.59,1,-6.4,0,0.02,0.02,0.9,0.16,0.08,170.0,rock
n3,Delta,Three,0.30,0.20,5,-9.4,1,0.12,0.52,0.1,0.26,0.58,90.0,rock
"""


def side_files():
    """The files every world holds beside its songs_data.bin (name -> text)."""
    seen = [f"t{i:04d}" for i in range(0, 600, 3)]
    return {
        "seen.txt": "\n".join(seen) + "\n",
        "seen_unknown.txt": "\n".join(seen[:50] + ["unknown-a", "unknown-b", "", "  t0003  ", "dupA"]) + "\n",
        "only.txt": "\n".join(f"t{i:04d}" for i in range(600) if i % 3) + "\n",
        "sample_seen.txt": "dupA\n\n  dupA  \nno-such-track\n",
        "priors.txt": "".join(f"{((i * 37) % 101) / 100:.2f}\n" for i in range(600)),
        "priors_short.txt": "0.5\n0.25\n",
        "priors_text.txt": "0.5\nhalf\n",
        "priors_range.txt": "".join("1.5\n" if i == 7 else "0.1\n" for i in range(600)),
    }


def environment():
    """The CLI's environment: no HIP device visible, so that the CPU backend answers on every host."""
    return dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def run(exe, argv, cwd, env=None, timeout=None):
    """The CLI as `recommender ARGV...` (argv[0], which the usage text prints, does not depend on where the tree lies)."""
    return subprocess.run(["recommender", *argv], executable=str(exe), capture_output=True, text=True, cwd=cwd, env=env, timeout=timeout)


def make_worlds(root, exe, env=None, only=None):
    """root/<world> for "sample" (tests/golden/sample_songs_data.bin), "c600" and "names" (each --preprocess'ed from its CSV here) and
    "empty" (no songs_data.bin); `only`: the worlds wanted.  Returns {world: directory}."""
    from tests.test_playlist_cpu import _write_csv
    worlds = {}
    for name in only or ("sample", "c600", "names", "empty"):
        d = worlds[name] = Path(root) / name
        d.mkdir()
        for fname, text in side_files().items():
            (d / fname).write_text(text)
        if name == "sample":
            shutil.copy(GOLD / "sample_songs_data.bin", d / "songs_data.bin")
        elif name == "c600":
            _write_csv(d / "songs.csv")
        elif name == "names":
            (d / "songs.csv").write_text(NAMES_CSV)
        if name in ("c600", "names"):
            p = run(exe, ["--preprocess", "songs.csv"], d, env)
            assert p.returncode == 0, p.stdout + p.stderr
    return worlds


PROGRESS = ("Loading preprocessed data", "Loaded ", "Initializing", "Operating in CPU fallback mode")
INITIALISER = ("Operating in CPU fallback mode", "[GPU Disabled]", "Falling back to CPU", "Successfully initialized with ", "[mi355rec]")


def without(text, prefixes):
    """text without the lines that start with one of `prefixes`."""
    return "".join(l for l in text.splitlines(keepends=True) if not l.startswith(prefixes))
