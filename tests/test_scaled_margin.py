"""The pre-filter of the scaled cosine requests (csrc/playlist_cut.hip.h, "SCALED"), checked on the CPU with a numpy model of
exactly the kernel's fp32 arithmetic against tests/scaled_oracle.py:

    q'_kj = fl(a_j q_kj),  |q'_k| = sqrtf(seq sum),  u_j = fl( fl(sum_k fl(w_k fl(q'_kj / |q'_k|))) / W )      (member order)
    abar_j = fl(a_j / a_max),  ubar_j = fl(abar_j u_j),  bn = |ubar|,  e = fl( fl(|abar| 1.001 / 254) + 8 ulp )
    den_floor = fl(2e-4 / fl(a_max min_k |q'_k|)),  l_floor = max(2^-6, den_floor),  gk_min = fl( fl(l_floor + e) (1 + 64 ulp) )
    margin_scaled = fl(4e-6 + fl((3 K + 64) ulp)),  c0 = fl(127 S fl(M + 16 ulp))
    per threshold:  tm = fl(T - margin_scaled),  base = fl( fl(tm / bn) 127 S ),  (fmul, fadd) = (1 - 16 ulp, -e) if tm >= 0 else (1 + 16 ulp, e)
    per row:        gk = fl( sqrt(seq sum_j fl(fl(abar_j k_j)^2)) / 127 ),  F = fl( fl(gk fmul) + fadd )
                    cut = int( clamp( fl( fl(base F) - c0 ), -2^30, 2^30 ) ) - 1
    a row is ruled out iff it is not special, gk >= gk_min and D(x) < cut(x)

with D the 8-bit replica's integer dot product for the query ubar and M its margin (tests/test_q8_margin.py).  The launch keeps
the pre-filter off unless a_max is in [2^-10, 8], den_floor <= 0.5, every |q'_k| and bn lie in [1.005e-4, 1e18] and bn >= 1e-3.
sqrt is the hardware's, good to one ulp: the model runs with the correctly rounded root and with both of its neighbours.
No row whose oracle score reaches T may ever be ruled out; and the bound is not vacuous."""
import numpy as np
import pytest

from tests.playlist_cut_model import F32, ScaledCut as Model
from tests.scaled_oracle import DROP3, EDGE, GENERAL, ONE, ONES, cosine_scores
from tests.test_q8_margin import q8_codes
from tests.weighted_oracle import weight_kinds

THREE = np.zeros(12, F32)
THREE[[0, 1, 9]] = 1                                          # three features kept: danceability, energy, valence


def scale_sets():
    top = (GENERAL * F32(8.0 / 3.0)).astype(F32)
    top[6] = 8
    low = (GENERAL * F32(2.0 ** -10 / 3.0)).astype(F32)
    low[6] = F32(2.0 ** -10)
    return {"ONES": ONES, "DROP3": DROP3, "GENERAL": GENERAL, "ONE": ONE, "EDGE": EDGE, "THREE": THREE, "a_max = 8": top, "a_max = 2^-10": low,
            "a_max above 8": (top * F32(1.001)).astype(F32), "a_max below 2^-10": (low * F32(0.999)).astype(F32)}


def catalogues(n):
    rng = np.random.default_rng(53)
    yield "uniform", rng.random((n, 12), dtype=F32)
    yield "signed gaussian", rng.normal(0.0, 1.0, (n, 12)).astype(F32)
    f = rng.random((n, 12), dtype=F32)
    f[::3, :] *= F32(1e-3)
    f[::3, [2, 4, 11]] = rng.random((len(f[::3]), 3), dtype=F32) * F32(5)          # mass only on key, mode, genre: L = 0 under DROP3
    f[1::3, [0, 1, 9]] *= F32(0.03)                                                # ... and rows about the floor of L under THREE
    yield "little mass on the kept features", f
    f = rng.normal(0.0, 1.0, (n, 12)).astype(F32)
    unit = (f / np.sqrt((f.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(F32)
    sizes = np.array([1.0049e-4, 1.0051e-4, 1.01e-4, 2e-4, 0.99e18, 1.01e18, 1.0, 1e3], F32)
    yield "norms at the edges of the valid range", (unit * sizes[rng.integers(0, len(sizes), size=n)][:, None]).astype(F32)


def member_sets(rng, f):
    n = f.shape[0]
    for k in (1, 3, 32):
        yield f"rows K={k}", np.nan_to_num(f[rng.integers(0, n, size=k)], nan=0.5, posinf=1.0, neginf=-1.0), k
        yield f"noise K={k}", rng.random((k, 12), dtype=F32), k
    d = rng.normal(0.0, 1.0, (3, 12)).astype(F32)
    for size in (1.01e-4, 3e-4, 1e-2):                                             # members just above the smallest valid norm
        yield f"tiny members {size}", (d / np.sqrt((d.astype(np.float64) ** 2).sum(axis=1, keepdims=True)) * size).astype(F32), 3


def thresholds(scores, topn=10):
    s = np.sort(scores[np.isfinite(scores)])[::-1]
    top = s[min(topn, s.size) - 1] if s.size else F32(0)
    return [F32(top), F32(0), F32(-0.3), F32(-1), F32(0.5), F32(s[s.size // 2]) if s.size else F32(0)]


def test_no_row_that_reaches_the_threshold_is_ruled_out():
    n = 6_000
    checked = off = ruled = 0
    on_by_set = {}
    for cname, f in catalogues(n):
        f = np.ascontiguousarray(f, F32)
        codes, valid = q8_codes(f)
        rng = np.random.default_rng([61, len(cname)])
        for mname, members, k in member_sets(rng, f):
            kinds = [("plain", None)] + list(weight_kinds(np.random.default_rng(k), k))
            for sname, a in scale_sets().items():
                for wname, w in (kinds if sname in ("DROP3", "GENERAL", "a_max = 8") else kinds[:1] + kinds[3:]):
                    mod = Model(codes, members, w, a)
                    if not mod.ok:
                        off += 1
                        continue
                    on_by_set[sname] = on_by_set.get(sname, 0) + 1
                    scores = cosine_scores(f, members, a, w)
                    for T in thresholds(scores):
                        for sqrt_ulps in (0, 1, -1):
                            out = mod.ruled_out(valid, T, sqrt_ulps)
                            bad = out & ~(scores < T)                              # (a NaN score is never below T)
                            assert not bad.any(), (cname, mname, sname, wname, float(T), sqrt_ulps, int(np.flatnonzero(bad)[0]))
                            ruled += int(out.sum())
                        checked += 1
    print(f"{checked} (catalogue, members, scales, weights, threshold) cases, {off} launches with the pre-filter off, {ruled} rows ruled "
          f"out; launches with the pre-filter on per scale set: {on_by_set}")
    assert checked > 1500 and ruled > 0 and off > 0
    assert "EDGE" not in on_by_set and "a_max above 8" not in on_by_set and "a_max below 2^-10" not in on_by_set
    assert all(on_by_set.get(s, 0) > 0 for s in ("ONES", "DROP3", "GENERAL", "ONE", "THREE", "a_max = 8", "a_max = 2^-10"))


@pytest.mark.parametrize("sname", ["DROP3", "ONES"])
def test_the_bound_is_not_vacuous(sname):
    """At the true top-10 threshold of 65 537 uniform rows at most 5 % survive, for K = 1, 3 and 32."""
    a = {"DROP3": DROP3, "ONES": ONES}[sname]
    n, topn = 65_537, 10
    f = np.random.default_rng(71).random((n, 12), dtype=F32)
    codes, valid = q8_codes(f)
    rng = np.random.default_rng(72)
    for k in (1, 3, 32):
        rows = rng.choice(n, size=k, replace=False)
        mod = Model(codes, f[rows], None, a)
        assert mod.ok
        scores = cosine_scores(f, f[rows], a)
        scores[rows] = -2                                                          # the member rows are excluded
        T = np.sort(scores)[::-1][topn - 1]
        out = mod.ruled_out(valid, T)
        assert not np.any(scores[out] >= T)
        survive = 1.0 - float(out.mean())
        print(f"{sname} K={k}: bn = {float(mod.bn):.4f}, M = {float(mod.margin):.5f}, T = {float(T):.5f}, survivors {100 * survive:.3f} %")
        assert survive <= 0.05, (sname, k, survive)
