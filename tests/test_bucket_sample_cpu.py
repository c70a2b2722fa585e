"""The host half of the 8-bit scan's bucketed sample (csrc/bucket_sample.h: ordering the base rows by (bucket, row) and cutting
the order into 2048-row regions), checked without a GPU: tests/bucket_sample_check.cpp is built with AddressSanitizer and UBSan
and run as its own process (nothing is preloaded into python) — its fixed cases (every row in one bucket, empty buckets, a base
that is not a multiple of 2048 rows, one region, the refusals) and random inputs held against numpy's stable sort."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "spotify_recommender_amd" / "csrc"
REGION = 2048


@pytest.fixture(scope="module")
def bucket_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bucket") / "bucket_sample_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           str(ROOT / "tests" / "bucket_sample_check.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def test_bucket_sample_h_under_sanitizers(bucket_check):
    p = subprocess.run([str(bucket_check)], capture_output=True, text=True)
    assert p.returncode == 0 and "bucket_sample.h: ok" in p.stdout, p.stdout + p.stderr


def _sort(exe, tmp_path, rows, bucket, n_buckets):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.asarray([rows.size, n_buckets], np.int64).tobytes() + rows.astype(np.int32).tobytes()
                    + bucket.astype(np.int32).tobytes())
    p = subprocess.run([str(exe), "sort", str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    out = np.frombuffer(dst.read_bytes(), dtype=np.int32)
    ok, regions = int(out[0]), int(out[1])
    return ok, regions, out[2:2 + regions * REGION], out[2 + regions * REGION:].reshape(regions, 2)


@pytest.mark.parametrize("m,n_buckets,used", [(2048, 1, 1), (3 * 2048, 64, 64), (2 * 2048 + 1, 64, 5), (2047, 1024, 1024),
                                              (7 * 2048 - 1, 300, 17), (1, 3, 3)])
def test_sort_against_numpy(bucket_check, tmp_path, m, n_buckets, used):
    """A permutation of the input in (bucket, row) order, the tail of the last region -1, and per region the buckets of its first and
    last real entry; `used` < n_buckets leaves buckets empty."""
    rng = np.random.default_rng([m, n_buckets])
    rows = np.sort(rng.choice(10 * m + 5, size=m, replace=False)).astype(np.int32)
    live = np.sort(rng.choice(n_buckets, size=used, replace=False))
    bucket = live[rng.integers(0, used, size=m)].astype(np.int32)
    ok, regions, got_rows, tab = _sort(bucket_check, tmp_path, rows, bucket, n_buckets)
    assert ok == 1 and regions == -(-m // REGION)
    order = np.lexsort((rows, bucket))   # by bucket, then row
    assert np.array_equal(got_rows[:m], rows[order]) and np.all(got_rows[m:] == -1)
    assert np.array_equal(np.sort(got_rows[:m]), rows)
    sorted_bucket = bucket[order]
    assert np.all(np.diff(sorted_bucket) >= 0)
    for g in range(regions):
        last = min((g + 1) * REGION, m) - 1
        assert tuple(tab[g]) == (sorted_bucket[g * REGION], sorted_bucket[last]), g


def test_sort_refuses_a_bucket_out_of_range(bucket_check, tmp_path):
    rows = np.arange(10, dtype=np.int32)
    bucket = np.zeros(10, dtype=np.int32)
    bucket[4] = 7
    ok, regions, got_rows, _ = _sort(bucket_check, tmp_path, rows, bucket, 7)
    assert ok == 0 and regions == 0 and got_rows.size == 0
