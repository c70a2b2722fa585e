"""The per-row cut of the playlist pre-filter with ROW PRIORS (csrc/playlist_cut.hip.h, "PRIOR"), checked on the CPU with a
numpy model of exactly the kernel's arithmetic against the oracle's exact ranking values:

    margin_prior = margin_mean + 96 * 2^-24                                   (margin_mean: tests/playlist_cut_model.model)
    base   = fl( fl( fl(T - margin_prior) / |u| ) * 127 S )                   (fp32; S = 32000)
    bs     = fl( fl(beta * 127 S) / |u| )
    cut(x) = int( clamp( fl(base - fl(p(x) bs)), -2^30, 2^30 ) ) - 1          (the conversion truncates towards zero)
    a row is ruled out iff D(x) < cut(x)

with D the 8-bit replica's integer dot product for the query u.  No valid row with v(x) = fl(s(x) + fl(beta p(x))) >= T may
ever be ruled out, for T of either sign and above 1; and the bound is not vacuous: at the true top-256 threshold of 65 537
uniform rows at most 5 % of the rows survive (the real-number model of the design gives at most 1.21 %; one launch-wide
max(beta p) would let 2 - 95 % through)."""
import numpy as np

from tests.playlist_cut_model import model, ruled_out
from tests.prior_oracle import blended, prior_kinds
from tests.test_q8_margin import q8_codes
from tests.weighted_oracle import weighted_scores


def hostile_priors(rng, n):
    tiny = (rng.random(n, dtype=np.float32) * np.float32(2e-38)).astype(np.float32)
    tiny[::3] = np.float32(1e-45)   # subnormals
    return {"+1": np.ones(n, np.float32), "-1": -np.ones(n, np.float32), "zero": np.zeros(n, np.float32), "tiny": tiny,
            "pm1": np.where(rng.random(n) < 0.5, np.float32(1), np.float32(-1)).astype(np.float32),
            "skewed": (rng.random(n, dtype=np.float32) ** 4).astype(np.float32)}


def playlists(rng, f):
    """(name, members, weights): K = 1, 3 and 32 likes, signed weights, and likes against dislikes with |u| near 1e-3."""
    n = f.shape[0]
    for k in (1, 3, 32):
        yield f"likes K={k}", f[rng.integers(0, n, size=k)], np.ones(k, np.float32)
    yield "signed K=5", f[rng.integers(0, n, size=5)], np.array([1.0, -0.5, 2.0, 0.25, -1.0], np.float32)
    a = f[int(rng.integers(0, n))]
    d = rng.normal(0.0, 1.0, 12).astype(np.float32)
    for eps in (2e-3, 4e-3, 8e-3, 2e-2):   # u = (a^ - b^) / 2: about eps / (2 |a|) long
        yield f"cancelling eps={eps}", np.stack([a, (a + np.float32(eps) * d).astype(np.float32)]), np.array([1.0, -1.0], np.float32)


def test_per_row_cut_never_rules_out_a_row_at_or_above_the_threshold():
    rng = np.random.default_rng(21)
    n = 20_000
    f = rng.random((n, 12), dtype=np.float32)
    f[5] = 0.0                       # a zero row (approx 0, score 0)
    f[6] = 1e-30                     # a special row: never ruled out
    codes, valid = q8_codes(f)
    small_u, negative_t, above_one, checked = 0, 0, 0, 0
    for name, members, w in playlists(rng, f):
        m = model(codes, valid, members, w)
        if m is None:
            continue
        D, un, mm = m
        small_u += un < 5e-3
        s = weighted_scores(f, members, w)
        for pname, p in hostile_priors(rng, n).items():
            for beta in (4.0, -4.0, 2.0 ** -20, -(2.0 ** -20), 0.25):
                v = blended(s, p, beta)
                order = np.sort(v)[::-1]
                for rank in (1, 10, 256, n // 2, n):
                    T = order[rank - 1]
                    out = ruled_out(D, valid, un, mm, T, beta, p)
                    assert not np.any(v[out] >= T), (name, pname, beta, rank, float(T), float(un))
                    negative_t += T < 0
                    above_one += T > 1
                    checked += 1
                # thresholds between and beyond the scores: the cut is safe for any T, not only for scores that occur
                for T in (np.float32(-5.0), np.float32(-1.5), np.float32(0.0), np.float32(1.5), np.float32(4.999), np.float32(5.5)):
                    out = ruled_out(D, valid, un, mm, T, beta, p)
                    assert not np.any(v[out] >= T), (name, pname, beta, float(T), float(un))
    print(f"{checked} thresholds checked; |u| < 5e-3 in {small_u} playlists; T < 0 {negative_t} times, T > 1 {above_one} times")
    assert small_u >= 1 and negative_t > 0 and above_one > 0, (small_u, negative_t, above_one)


def test_per_row_cut_is_not_vacuous():
    rng = np.random.default_rng(22)
    n, topn = 65_537, 256
    f = rng.random((n, 12), dtype=np.float32)
    codes, valid = q8_codes(f)
    pri = prior_kinds(rng, n)
    worst = 0.0
    for k in (1, 3, 32):
        members = f[rng.integers(0, n, size=k)]
        w = np.ones(k, np.float32)
        m = model(codes, valid, members, w)
        assert m is not None, k
        D, un, mm = m
        s = weighted_scores(f, members, w)
        for pname, p in pri.items():
            for beta in (0.25, 1.0, -0.5, 4.0):
                v = blended(s, p, beta)
                T = np.sort(v)[::-1][topn - 1]
                out = ruled_out(D, valid, un, mm, T, beta, p)
                assert not np.any(v[out] >= T), (k, pname, beta)
                survive = 1.0 - float(out.mean())
                print(f"K={k:2d} {pname:8s} beta={beta:5.2f}  |u|={float(un):.4f}  survivors {100 * survive:.2f} %")
                worst = max(worst, survive)
                assert survive <= 0.05, (k, pname, beta, survive)
    print(f"worst share of rows sent to the exact chains: {100 * worst:.2f} %")
