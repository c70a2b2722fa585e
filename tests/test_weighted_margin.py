"""The error bound of the WEIGHTED playlist pre-filter (csrc/playlist_cut.hip.h, "PLAIN"), checked on the CPU with a numpy model of
exactly that arithmetic against the weighted oracle's exact scores:

    |q_k| = the chain's fp32 norm,  W = fl(sum_k |w_k|),  u_j = fl(sum_k fl(w_k fl(q_kj / |q_k|))) / W   (fp32, member order)
    approx = the 8-bit replica's D / (127 S) for the query u (tests/test_q8_margin.py), M = its per-query margin
    margin_mean = |u| M + 4e-6 + (3K + 32) 2^-24

for every valid row and every playlist the kernel claims the bound for: |score(x) - |u| approx| <= margin_mean.  A
playlist is left out ONLY where the kernel itself turns the pre-filter off (a member norm out of [1.005e-4, 1e18],
|u| < 1e-3 or not finite, q8 digits refused), and at least 80 % of the generated playlists must be claimed, so the test
cannot pass by claiming nothing.  It also checks that the bound is not vacuous and that the integer cutoff derived from a
threshold T (of either sign) never rules out a row whose score is >= T."""
import numpy as np

from tests.playlist_cut_model import model, weighted_direction
from tests.test_batched_margin import catalogues
from tests.test_q8_margin import DOT_SCALE, q8_codes, q8_threshold
from tests.weighted_oracle import weight_kinds, weight_sum, weighted_scores

KS = (1, 2, 5, 10, 32)


def test_weighted_prefilter_error_stays_inside_the_margin_and_the_cutoff_is_safe():
    rng = np.random.default_rng(5)
    n = 40_000
    worst, claimed, generated, ruled_out = 0.0, 0, 0, []
    by_kind = {}
    for name, f in catalogues(rng, n):
        f = np.ascontiguousarray(f, dtype=np.float32)
        codes, valid = q8_codes(f)
        for k in KS:
            members = f[rng.integers(0, n, size=k)]
            for kind, w in weight_kinds(rng, k):
                generated += 1
                m = model(codes, valid, members, w)
                if m is None:
                    continue
                D, un, mm = m
                approx = (D.astype(np.float32) * (np.float32(1) / DOT_SCALE)).astype(np.float32).astype(np.float64)
                exact32 = weighted_scores(f, members, w)
                err = np.abs(exact32.astype(np.float64) - float(un) * approx)[valid]
                if not err.size:
                    continue
                claimed += 1
                by_kind[kind] = by_kind.get(kind, 0) + 1
                ratio = float(err.max()) / mm
                print(f"{name:34s} K={k:2d} {kind:9s} |u|={float(un):.4f} margin={mm:.3e} worst error={float(err.max()):.3e} ({ratio:.3f})")
                worst = max(worst, ratio)
                assert err.max() <= mm, (name, k, kind, float(err.max()), mm)
                order = np.sort(exact32)[::-1]
                for topk in (1, 10, 100, 1000):
                    T = order[topk - 1]
                    cut = q8_threshold(np.float32((np.float32(T) - np.float32(mm)) / un))
                    out = valid & (D < cut)
                    assert not np.any(exact32[out] >= T), (name, k, kind, topk)
                    if topk == 10 and name == "uniform":
                        ruled_out.append((kind, k, float(out.mean())))
    print(f"claimed {claimed} of {generated} playlists, worst error / margin {worst:.3f}; ruled out on uniform: {ruled_out}")
    assert claimed >= 0.8 * generated, (claimed, generated)
    assert set(by_kind) == {"positive", "signed", "dislikes"}, by_kind
    # not vacuous: the quantisation error realises a good part of the margin somewhere, and never exceeds it
    assert 0.3 < worst <= 1.0, worst
    # and the filter does rule rows out (the point of it) for likes-only playlists of a uniform catalogue
    assert all(frac > 0.3 for kind, k, frac in ruled_out if kind == "positive" and k <= 10), ruled_out


def test_all_ones_is_the_unweighted_model_and_scores():
    """Identity 1 in the model: weights of 1.0 give the unweighted kernel's u bit for bit and the plain mean's scores."""
    from tests.playlist_oracle import mean_scores
    from tests.playlist_cut_model import mean_direction
    rng = np.random.default_rng(6)
    for name, f in catalogues(rng, 5_000):
        f = np.ascontiguousarray(f, dtype=np.float32)
        for k in KS:
            members = f[rng.integers(0, f.shape[0], size=k)]
            ones = np.ones(k, np.float32)
            assert weight_sum(ones) == np.float32(k)
            u0, un0, ok0 = mean_direction(members)
            u1, un1, ok1 = weighted_direction(members, ones)
            assert ok0 == ok1 and np.array_equal(u0.view(np.uint32), u1.view(np.uint32)), (name, k)
            a, b = mean_scores(f, members), weighted_scores(f, members, ones)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, k)
            for p in (8, -8):      # identity 2: a power of two changes nothing
                c = weighted_scores(f, members, ones * np.float32(2.0 ** p))
                assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), (name, k, p)
