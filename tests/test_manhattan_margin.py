"""The pre-filter of the MANHATTAN REQUESTS (csrc/playlist_cut.hip.h, "MANHATTAN"), checked on the CPU with
tests/manhattan_cut_model.py — a numpy mirror of the kernel's arithmetic, operation for operation — against
tests/manhattan_oracle.py: the catalogue families of tests/test_distance_margin.py (uniform, tied, duplicated, signed wide, one
dominant raw feature, norms at the edges of the valid range), K = 1, 3, 32, members taken from the rows and from noise, T at the
true thresholds, 0, far above and +inf.  No row with m(x) <= T may ever be ruled out; and the bound is not vacuous: at the true
top-10 threshold of 65 537 uniform rows at most 2 % of the rows survive for each K (the cap the any-of cut is held to; the
real-number model of the per-member bound leaves 0.03 - 0.12 %).  Shares the kernel's own arithmetic leaves, as printed by the
second test: K = 1: 0.023 - 0.035 %, K = 3: 0.055 - 0.066 %, K = 32: 0.114 - 0.130 %."""
import numpy as np

from tests.manhattan_cut_model import ManhattanCut as Model
from tests.manhattan_oracle import mean_l1
from tests.playlist_cut_model import stored_norms
from tests.playlist_sweep_cases import catalogue_of_kind
from tests.test_distance_margin import catalogues, thresholds
from tests.test_q8_margin import q8_codes


def member_sets(rng, f):
    n = f.shape[0]
    for k in (1, 3, 32):
        yield f"rows K={k}", np.nan_to_num(f[rng.integers(0, n, size=k)], nan=0.5, posinf=1.0, neginf=-1.0)
        yield f"noise K={k}", rng.random((k, 12), dtype=np.float32)
    yield "zero and tiny members", np.stack([np.zeros(12, np.float32), np.full(12, 1e-30, np.float32), f[0]])
    yield "a member beyond the claimed range", np.stack([f[0], np.full(12, 1e18, np.float32)])   # |q| = 3.5e18: the cut is off


def test_no_row_at_or_below_the_threshold_is_ruled_out():
    n = 20_000
    checked, off, ruled = 0, 0, 0
    for cname, f in catalogues(n):
        f = np.ascontiguousarray(f, np.float32)
        rng = np.random.default_rng([43, len(cname)])
        codes, valid = q8_codes(f)
        s = stored_norms(f)
        for mname, members in member_sets(rng, f):
            mod = Model(codes, members)
            if not mod.ok:
                off += 1
                continue
            m = mean_l1(f, members)
            acc = mod.lower_sum(s)
            for T in thresholds(m):
                out = mod.ruled_out(valid, s, T, acc)
                assert not np.any(m[out] <= T), (cname, mname, float(T))
                ruled += int(out.sum())
                checked += 1
    print(f"{checked} (catalogue, members, threshold) cases, {off} launches with the pre-filter off, {ruled} rows ruled out")
    # (off: the member beyond the range in each of the six catalogues, and row sets that hold a row of norm 1.01e18)
    assert checked > 300 and ruled > 0 and 6 <= off <= 9


def test_the_bound_is_not_vacuous():
    """At the true top-10 threshold at most 2 % of 65 537 uniform rows survive, for K = 1, 3, 32 (members by row, excluded)."""
    n, topn = 65_537, 10
    f = catalogue_of_kind(0, n)
    codes, valid = q8_codes(f)
    s = stored_norms(f)
    rng = np.random.default_rng(44)
    for k in (1, 3, 32):
        for trial in range(3):
            rows = rng.choice(n, size=k, replace=False)
            members = f[rows]
            mod = Model(codes, members)
            assert mod.ok
            m = mean_l1(f, members)
            m[rows] = np.inf                                                               # the member rows are excluded
            T = np.sort(m)[topn - 1]
            out = mod.ruled_out(valid, s, T)
            assert not np.any(m[out] <= T)
            survive = 1.0 - float(out.mean())
            print(f"K = {k}, trial {trial}: T = {float(T):.5f}, survivors {100 * survive:.4f} %")
            assert survive <= 0.02, (k, trial, survive)


def test_the_mirror_holds_the_constants_the_kernel_is_compiled_from():
    """Drift guard: the constants of csrc/playlist_cut.hip.h ("MANHATTAN") and of the prologue in csrc/anyof.hip.h, read from the
    source text, are the ones tests/manhattan_cut_model.py computes with."""
    import re

    from spotify_recommender_amd import build
    from tests import manhattan_cut_model as mirror
    cut = (build.CSRC / "playlist_cut.hip.h").read_text()
    scan = (build.CSRC / "anyof.hip.h").read_text()
    a, b, c = re.search(r"constexpr float kL1HalfSteps = ([0-9.]+)f \* ([0-9.]+)f / ([0-9.]+)f;", cut).groups()
    assert np.float32(np.float32(np.float32(a) * np.float32(b)) / np.float32(c)) == mirror.HALF_STEPS
    m, add = re.search(r"playlist_cut_l1_eps\(int k\) \{ return static_cast<float>\((\d+) \* k \+ (\d+)\) \* kPlUlp; \}", cut).groups()
    assert re.search(r"constexpr float kPlUlp = 5\.9604645e-8f;", cut) and np.float32(5.9604645e-8) == mirror.ULP
    for k in (1, 3, 32):
        mod = Model(np.zeros((1, 12), np.int64), np.zeros((k, 12), np.float32))
        assert mod.ce == np.float32(np.float32(1.0) - np.float32(np.float32(int(m) * k + int(add)) * mirror.ULP))
        assert mod.ke1 == np.float32(np.float32(k) * mirror.HALF_STEPS)
    assert "sm.l1[0] = 1.0f - playlist_cut_l1_eps(k);" in scan and "sm.l1[1] = static_cast<float>(k) * kL1HalfSteps;" in scan
    assert "sc[r] = s4[r] * (1.0f / 127.0f);" in cut and "acc[r] * ce > s4[r] * ke1 + kt" in cut
    assert "kBqMinNorm = 1.005e-4f" in (build.CSRC / "batched.hip.h").read_text() and mirror.MIN_NORM == np.float32(1.005e-4)
    assert "kBqMaxNorm = 1e18f" in (build.CSRC / "batched.hip.h").read_text() and mirror.MAX_NORM == np.float32(1e18)
