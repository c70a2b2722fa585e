"""The pre-filter of the DISTANCE REQUESTS (csrc/playlist_cut.hip.h, "DISTANCE"), checked on the CPU with a numpy model of exactly
the kernel's arithmetic against tests/distance_oracle.py:

    c_j  = fl( fl(q_0j + ... + q_{K-1}j) / K ),  |c| = sqrtf(seq sum c_j^2)            (fp32, member order)
    Q2   = fl( fl(|q_0|^2 + ... + |q_{K-1}|^2) / K ),  |q_k|^2 the sequential fp32 sum of squares
    eps  = (4 K + 128) 2^-24
    q2e  = fl(Q2 fl(1 - eps));   s2c = fl(127 S / fl(2 |c|));   a1 = fl(s2c fl(1 - eps));   c0 = fl(127 S fl(M + eps))
    b(T) = fl( fl(q2e - T) s2c )                                                       (refreshed when the threshold moves)
    cut(x) = int( clamp( fl( fl( fl(a1 s) + fl(b rcp(s)) ) - c0 ), -2^30, 2^30 ) ) - 1,   s = the row's stored norm
    a row is ruled out iff it is not special, s lies in [1.005e-4, 1e18] and D(x) < cut(x)

with D the 8-bit replica's integer dot product for the query c and M its margin (tests/test_q8_margin.py).  rcp is the
hardware's reciprocal, good to one ulp: the model is run with the correctly rounded reciprocal and with both of its
neighbours.  No row with m(x) <= T may ever be ruled out; and the bound is not vacuous."""
import numpy as np

from tests.distance_oracle import mean_sqdist
from tests.playlist_cut_model import DistanceCut as Model, stored_norms
from tests.playlist_sweep_cases import catalogue_of_kind
from tests.test_q8_margin import q8_codes


def catalogues(n):
    yield "uniform", catalogue_of_kind(0, n)
    yield "mass ties", catalogue_of_kind(1, n)
    yield "duplicates", catalogue_of_kind(5, n)
    yield "signed wide", catalogue_of_kind(3, n)
    rng = np.random.default_rng(31)
    f = rng.random((n, 12), dtype=np.float32)
    f[:, 10] = (60 + 140 * rng.random(n)).astype(np.float32)                              # an unnormalised tempo
    yield "one dominant feature", f
    f = rng.random((n, 12), dtype=np.float32)
    unit = (f / np.sqrt((f.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)
    scales = np.array([1.0049e-4, 1.0051e-4, 1.01e-4, 1.0e-4, 0.99e18, 1.01e18, 1.0, 1e3], np.float32)
    yield "norms at the edges of the valid range", (unit * scales[rng.integers(0, len(scales), size=n)][:, None]).astype(np.float32)


def member_sets(rng, f):
    n = f.shape[0]
    for k in (1, 3, 32):
        yield f"rows K={k}", np.nan_to_num(f[rng.integers(0, n, size=k)], nan=0.5, posinf=1.0, neginf=-1.0)
        yield f"noise K={k}", rng.random((k, 12), dtype=np.float32)
    a = rng.random(12, dtype=np.float32)
    d = rng.normal(0.0, 1.0, 12).astype(np.float32)
    for tiny in (1e-2, 1e-3, 3e-4, 1e-5):                                                 # a centroid about `tiny` long
        yield f"tiny centroid {tiny}", np.stack([a, (-a + np.float32(2 * tiny) * d).astype(np.float32)])


def thresholds(m):
    fin = np.sort(m[np.isfinite(m)])
    out = [fin[min(r, fin.size) - 1] for r in (1, 10, 256, fin.size // 2, fin.size)] if fin.size else []
    top = fin[-1] if fin.size else np.float32(1)
    return out + [np.float32(0), np.float32(min(float(top) * 1e6 + 1e6, 3e38)), np.float32(np.inf)]


def test_no_row_at_or_below_the_threshold_is_ruled_out():
    n = 20_000
    checked, off, ruled = 0, 0, 0
    for cname, f in catalogues(n):
        f = np.ascontiguousarray(f, np.float32)
        rng = np.random.default_rng([41, len(cname)])
        codes, valid = q8_codes(f)
        s = stored_norms(f)
        for mname, members in member_sets(rng, f):
            mod = Model(codes, members)
            if not mod.ok:
                off += 1
                continue
            m = mean_sqdist(f, members)
            for T in thresholds(m):
                for rcp_ulps in (0, 1, -1):
                    out = mod.ruled_out(valid, s, T, rcp_ulps)
                    assert not np.any(m[out] <= T), (cname, mname, float(T), rcp_ulps, float(mod.cn))
                    ruled += int(out.sum())
                checked += 1
    print(f"{checked} (catalogue, members, threshold) cases, {off} launches with the pre-filter off, {ruled} rows ruled out")
    assert checked > 300 and ruled > 0 and 0 < off < 20


def test_the_bound_is_not_vacuous():
    """At the true top-10 threshold, k = 1, at most 1 % of 65 537 uniform rows survive (the real-number model gives 0.05 %)."""
    n, topn = 65_537, 10
    f = catalogue_of_kind(0, n)
    codes, valid = q8_codes(f)
    s = stored_norms(f)
    rng = np.random.default_rng(42)
    for trial in range(4):
        row = int(rng.integers(0, n))
        members = f[row:row + 1]
        mod = Model(codes, members)
        assert mod.ok
        m = mean_sqdist(f, members)
        m[row] = np.inf                                                                    # the member row is excluded
        T = np.sort(m)[topn - 1]
        out = mod.ruled_out(valid, s, T)
        assert not np.any(m[out] <= T)
        survive = 1.0 - float(out.mean())
        print(f"query row {row}: |c| = {float(mod.cn):.4f}, M = {float(mod.margin):.5f}, T = {float(T):.5f}, survivors {100 * survive:.3f} %")
        assert survive <= 0.01, (row, survive)
