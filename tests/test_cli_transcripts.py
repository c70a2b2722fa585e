"""The drop-in CLI (csrc/main.cpp) against tests/golden/cli_transcripts.json.gz: what the CLI of the commit BEFORE the one-path
refactor of the class and the CLI printed for some three hundred command lines (every option alone and in pairs under --song, --id
and --playlist, every refusal, every malformed value; recorded by tests/golden/make_cli_transcripts.py on that commit).

On the CPU backend every case is replayed: a run that exits 0 must give the same bytes on stdout and stderr; a run that does not
must give the same exit code and stderr, and the same stdout once the loader's and the initialiser's progress lines are left out
(a refused run may be refused before or after the catalogue is opened).  On the GPU twelve cases, one per request shape, are
replayed and compared without the initialiser's own lines: the ids, scores and distances printed are bit for bit those of the CPU
backend."""
import signal
import subprocess

import pytest

from tests import cli_transcripts as T


@pytest.fixture(scope="module")
def cases():
    return T.load_cases()


@pytest.fixture(scope="module")
def cli(engine_lib):
    from spotify_recommender_amd import build
    build.build_shim()
    return build.BIN_CLI


def test_fixture_is_smaller_than_the_largest_one_committed(golden_dir, cases):
    unpacked = len(T.dump_cases(cases))                                                      # (the JSON the recorder packs)
    assert T.FIXTURE.stat().st_size < unpacked < (golden_dir / "catalogue4096.npz").stat().st_size
    assert sum(1 for c in cases if c.get("gpu")) == 12


def test_cli_prints_what_it_printed_before_the_refactor(cli, cases, tmp_path):
    env = T.environment()
    worlds = T.make_worlds(tmp_path, cli, env)
    wrong = []
    for case in cases:
        cwd = worlds[case["world"]]
        if case["argv"][:1] == ["--preprocess"]:
            (cwd / "songs_data.bin").unlink(missing_ok=True)        # (the case writes it again)
        p = T.run(cli, case["argv"], cwd, env)
        got, want = (p.returncode, p.stdout, p.stderr), (case["exit"], case["stdout"], case["stderr"])
        if case["exit"] != 0:
            got, want = ((e, T.without(out, T.PROGRESS), err) for e, out, err in (got, want))
        if got != want:
            wrong.append((case["argv"], got, want))
    assert not wrong, f"{len(wrong)} of {len(cases)} command lines differ; the first: {wrong[0]}"


@pytest.mark.gpu
def test_cli_on_the_gpu_prints_the_recorded_ids_and_values(cli, cases, tmp_path):
    worlds = T.make_worlds(tmp_path, cli, T.environment(), only=("c600",))     # (--preprocess needs no device)
    for case in (c for c in cases if c.get("gpu")):
        try:
            p = T.run(cli, case["argv"], worlds[case["world"]], timeout=60)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{case['argv']}: no answer within its time limit; nothing more is started")
        assert p.returncode >= 0, f"{case['argv']}: ended by {signal.Signals(-p.returncode).name}; nothing more is started"
        assert "Successfully initialized with 600 songs on GPU" in p.stdout, p.stdout + p.stderr
        got = (p.returncode, T.without(p.stdout, T.INITIALISER), T.without(p.stderr, T.INITIALISER))
        want = (case["exit"], T.without(case["stdout"], T.INITIALISER), T.without(case["stderr"], T.INITIALISER))
        assert got == want, case["argv"]
