"""The error bound of the playlist pre-filter (csrc/playlist_cut.hip.h, "PLAIN"), checked on the CPU with a numpy model of exactly that
arithmetic against the oracle's exact mean scores:

    |q_k| = the chain's fp32 norm,  u_j = fl(sum_k fl(q_kj / |q_k|)) / K   (fp32, member order),  |u| in fp32
    approx = the 8-bit replica's D / (127 S) for the query u (tests/test_q8_margin.py), M = its per-query margin
    margin_mean = |u| M + 4e-6 + (2K + 32) 2^-24

for every valid row (|r|^2 in [1.01e-8, 1e36]) and every playlist the kernel claims the bound for (every |q_k| in
[1.005e-4, 1e18], |u| >= 1e-3): |score(x) - |u| approx| <= margin_mean.  The test also checks that the bound is not
vacuous, and that the integer cutoff the kernel derives from a threshold T never rules out a row whose mean is >= T."""
import numpy as np

from oracle import oracle
from tests.playlist_cut_model import unweighted_model as model
from tests.playlist_oracle import mean_scores
from tests.test_batched_margin import catalogues
from tests.test_q8_margin import DOT_SCALE, q8_threshold


def playlists(rng, f):
    n = f.shape[0]
    for k in (1, 2, 5, 10, 32):
        yield f[rng.integers(0, n, size=k)]
        yield rng.random((k, 12), dtype=np.float32) * np.float32(10.0 ** rng.integers(-3, 4))
        yield rng.normal(0, 1, (k, 12)).astype(np.float32)
    yield np.repeat(f[rng.integers(0, n, size=1)], 4, axis=0)        # duplicates
    base = rng.random(12, dtype=np.float32)
    yield np.stack([base, -base + np.float32(1e-2), base * 3])       # nearly cancelling pair


def test_mean_prefilter_error_stays_inside_the_margin():
    rng = np.random.default_rng(2027)
    n = 40_000
    worst = 0.0
    claimed = 0
    for name, f in catalogues(rng, n):
        f = np.ascontiguousarray(f, dtype=np.float32)
        for members in playlists(rng, f):
            m = model(f, members)
            if m is None:
                continue
            D, valid, un, mm = m
            approx = (D.astype(np.float32) * (np.float32(1) / DOT_SCALE)).astype(np.float32).astype(np.float64)
            exact = mean_scores(f, members).astype(np.float64)
            err = np.abs(exact - float(un) * approx)[valid]
            if err.size:
                claimed += 1
                worst = max(worst, float(err.max()) / mm)
                assert err.max() <= mm, (name, len(members), float(err.max()), mm)
    assert claimed > 20
    # not vacuous: the quantisation error realises a good part of the margin somewhere, and never exceeds it
    assert 0.3 < worst <= 1.0, worst


def test_integer_cutoff_never_rules_out_a_row_at_or_above_the_threshold():
    rng = np.random.default_rng(8)
    f = np.ascontiguousarray(oracle.mt19937_uniform(8, 50_000))
    for members in playlists(rng, f):
        m = model(f, members)
        if m is None:
            continue
        D, valid, un, mm = m
        exact = mean_scores(f, members)
        for topk in (1, 10, 100, 1000):
            T = np.sort(exact)[::-1][topk - 1]
            cut = q8_threshold(np.float32((np.float32(T) - np.float32(mm)) / un))
            out = valid & (D < cut)
            assert not np.any(exact[out] >= T), (len(members), topk)
            # and the filter does rule rows out (the point of it) where the playlist has a direction
            if topk == 10 and len(members) <= 10:
                assert out.mean() > 0.3, out.mean()
