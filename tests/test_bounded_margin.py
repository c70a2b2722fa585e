"""The two cuts of the count launch (csrc/playlist_cut.hip.h, "BOUNDED"), checked on the CPU with tests/bounded_cut_model.py (a numpy
mirror of exactly that arithmetic) against the oracle's exact mean scores: no row the mirror PROVES IN scores below the floor, no row
at or above the floor is RULED OUT, on the catalogues and member sets of tests/test_playlist_margin.py and tests/test_anyof_margin.py,
with |u| near 1e-3, negative floors and floors above 1; and the band of rows that neither cut decides is not vacuous."""
import numpy as np

from tests.bounded_cut_model import NEVER, BoundedCut
from tests.bounded_oracle import image
from tests.playlist_oracle import mean_scores
from tests.test_anyof_margin import catalogues as anyof_catalogues, member_sets
from tests.test_batched_margin import catalogues
from tests.test_playlist_margin import playlists


def _floors(exact, valid):
    s = np.sort(exact[valid])
    picks = [s[0], s[len(s) // 100], s[len(s) // 4], s[len(s) // 2], s[-len(s) // 4], s[-100], s[-10], s[-1]] if s.size > 200 else list(s[:3])
    fixed = [-3e38, -2.5, -1.0, -0.5, -1e-3, -0.0, 0.0, 1e-3, 0.5, 0.9999, 1.0, 1.0000001, 1.5, 2.5, 3e38]
    out = [np.float32(x) for x in fixed + picks]
    return out + [np.nextafter(x, np.float32(4)) for x in picks] + [np.nextafter(x, np.float32(-4)) for x in picks]


def _check(name, f, members):
    cut = BoundedCut(f, members)
    if not cut.ok:
        return 0
    exact = mean_scores(f, members)
    for b in _floors(exact, cut.valid):
        matches = image(exact) >= image(b)
        proven, out = cut.proven_in(b), cut.ruled_out(b)
        assert not np.any(proven & ~matches), (name, len(members), float(b), "a row proven in scores below the floor")
        assert not np.any(out & matches), (name, len(members), float(b), "a row at or above the floor is ruled out")
        assert not np.any(proven & out)
    return 1


def test_no_row_proven_in_scores_below_the_floor_and_none_at_or_above_it_is_ruled_out():
    rng = np.random.default_rng(2032)
    claimed = 0
    for name, f in catalogues(rng, 20_000):
        f = np.ascontiguousarray(f, dtype=np.float32)
        for members in playlists(rng, f):
            claimed += _check(name, f, members)
    for name, f in anyof_catalogues(rng, 20_000):
        for k in (1, 3, 32):
            for what, members in member_sets(rng, f, k):
                claimed += _check(f"{name}, {what}", f, members)
    assert claimed > 40, claimed


def test_mean_directions_near_the_switch_off_norm():
    """|u| near 1e-3 (kPlMinMeanNorm): members that nearly cancel.  Where the kernel still claims the bound both cuts hold; the
    quotient (T +- margin) / |u| is then beyond +-2 for most floors and the clamps must fail safe."""
    rng = np.random.default_rng(77)
    f = rng.normal(0, 1, (20_000, 12)).astype(np.float32)
    claimed = 0
    for eps in (8e-4, 1.0e-3, 1.1e-3, 2e-3, 5e-3, 2e-2):
        base = rng.normal(0, 1, 12).astype(np.float32)
        base /= np.float32(np.linalg.norm(base))
        members = np.stack([base, (-base + np.float32(2 * eps) * rng.normal(0, 1, 12).astype(np.float32)).astype(np.float32)])
        cut = BoundedCut(f, members)
        if cut.ok:
            assert cut.un < 0.2
            claimed += _check(f"cancelling pair {eps}", f, members)
    assert claimed >= 3, claimed


def test_the_clamps_fail_safe():
    rng = np.random.default_rng(5)
    f = rng.random((5_000, 12), dtype=np.float32)
    cut = BoundedCut(f, f[:3])
    assert cut.ok
    assert cut.cuts(np.float32(3e38))[1] == NEVER and cut.cuts(np.float32(2.5))[1] == NEVER      # a quotient of 2 or more proves nothing
    assert not cut.proven_in(np.float32(1.5)).any() and cut.ruled_out(np.float32(1.5))[cut.valid].all()
    assert cut.proven_in(np.float32(-3e38))[cut.valid].all() and not cut.ruled_out(np.float32(-3e38)).any()


def test_not_vacuous_at_the_median_floor():
    """The cap is a condition: of 65 537 uniform rows, members drawn from the rows, at the median score at most 20 % (K = 1), 25 % (K = 3)
    and 30 % (K = 32) are neither proven in nor ruled out.  (A float64 model of the margin gives 11.8, 16.6 and 22.3 %.)  The fp32
    mirror's own figures are printed."""
    n = 65_537
    f = np.random.default_rng(5).random((n, 12)).astype(np.float32)
    rng = np.random.default_rng(6)
    for k, cap in ((1, 0.20), (3, 0.25), (32, 0.30)):
        members = f[rng.choice(n, size=k, replace=False)]
        cut = BoundedCut(f, members)
        assert cut.ok
        exact = mean_scores(f, members)
        b = np.float32(np.median(exact))
        proven, out = cut.proven_in(b), cut.ruled_out(b)
        undecided = float(np.mean(~proven & ~out))
        print(f"K = {k}: proven in {proven.mean():.3%}, ruled out {out.mean():.3%}, undecided {undecided:.3%}")
        matches = image(exact) >= image(b)
        assert not np.any(proven & ~matches) and not np.any(out & matches)
        assert undecided <= cap, (k, undecided)
