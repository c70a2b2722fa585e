"""The ANY-OF pre-filter (csrc/playlist_cut.hip.h, "ANY") on the CPU: tests/anyof_cut_model.py, the numpy mirror of its arithmetic,
against tests/anyof_oracle.py.  SOUNDNESS: no row with v(x) >= T is ruled out, whatever T.  NOT VACUOUS: at the true top-10
threshold of 65 537 uniform rows at most 2 % of the rows survive (a condition, not a measurement; the figures are printed)."""
import numpy as np

from oracle import oracle
from tests.anyof_cut_model import AnyCut
from tests.anyof_oracle import value

MIN_NORM, MAX_NORM = np.float32(1.005e-4), np.float32(1e18)


def catalogues(rng, n):
    u = rng.random((n, 12), dtype=np.float32)
    yield "uniform", u
    yield "signed", rng.normal(0, 1, (n, 12)).astype(np.float32)
    t = u.copy()
    t[n // 2:] = t[: n - n // 2]                                         # every row twice: ties
    t[:50] = t[0]                                                        # fifty duplicates of one row
    yield "tied and duplicated", t
    e = u.copy()                                                         # norms at the edges of the valid range, and just outside
    for i, s in enumerate((1.0e-4, 1.005e-4, 1.01e-4, 1.1e-4, 1e17, 9.9e17, 1e18, 1.1e18, 1e-30, 0.0)):
        d = e[i] / np.float32(np.sqrt(np.sum(e[i].astype(np.float64) ** 2)))
        e[i] = (d * np.float32(s)).astype(np.float32)
    yield "norms at the edges", e


def member_sets(rng, f, k):
    n = f.shape[0]
    yield "rows", f[rng.choice(n, size=k, replace=False)]
    yield "uniform", rng.random((k, 12), dtype=np.float32)
    yield "signed", rng.normal(0, 1, (k, 12)).astype(np.float32)
    m = rng.random((k, 12), dtype=np.float32)
    for i, s in enumerate((1.006e-4, 9.9e17, 2e-4)[:k]):                 # members with norms at the edges of the valid range
        d = m[i] / np.float32(np.sqrt(np.sum(m[i].astype(np.float64) ** 2)))
        m[i] = (d * np.float32(s)).astype(np.float32)
    yield "edge norms", m
    if k > 1:
        d = rng.random((k, 12), dtype=np.float32)
        d[1] = d[0]                                                      # a duplicated member
        yield "duplicated member", d


def test_no_row_at_or_above_the_threshold_is_ruled_out():
    rng = np.random.default_rng(2031)
    n = 20_000
    claimed = ruled = 0
    for name, f in catalogues(rng, n):
        f = np.ascontiguousarray(f, np.float32)
        for k in (1, 3, 32):
            for what, members in member_sets(rng, f, k):
                cut = AnyCut(f, members)
                if not cut.ok:
                    continue
                claimed += 1
                v, _ = value(f, members)
                top10 = np.sort(v)[::-1][9]
                for T in (top10, np.float32(0.0), np.float32(-0.0), np.float32(-0.3), np.float32(-1.0), np.float32(0.5), np.float32(1.0)):
                    out = cut.ruled_out(T)
                    ruled += int(out.sum())
                    assert not np.any(v[out] >= T), (name, k, what, float(T), int(np.sum(v[out] >= T)))
    assert claimed >= 40 and ruled > 0


def test_the_cut_is_off_where_a_member_is_not_claimed():
    rng = np.random.default_rng(5)
    f = rng.random((1000, 12), dtype=np.float32)
    good = rng.random((3, 12), dtype=np.float32)
    assert AnyCut(f, good).ok
    for bad in (0.0, 1e-30, 1e-5, 1e19, np.nan, np.inf):
        m = good.copy()
        m[2] = np.float32(bad)
        with np.errstate(all="ignore"):                              # (1e19 squared overflows fp32: that is the case)
            assert not AnyCut(f, m).ok, bad


def test_not_vacuous_at_the_true_top10_threshold():
    """The cap is a condition: at most 2 % of the rows survive.  The fp32 mirror's own figures are printed."""
    n = 65537
    f = np.ascontiguousarray(oracle.mt19937_uniform(700 + n % 89, n))
    rng = np.random.default_rng(1)
    for k in (1, 3, 32):
        rows = rng.choice(n, size=k, replace=False)
        members = f[rows]
        cut = AnyCut(f, members)
        assert cut.ok
        v, _ = value(f, members)
        T = np.sort(np.delete(v, rows))[::-1][9]             # (as a request by row ranks: the member rows themselves left out)
        out = cut.ruled_out(T)
        assert not np.any(v[out] >= T)
        survive = 1.0 - out.mean()
        print(f"any-of cut, K = {k}: {100 * survive:.3f} % of {n} rows survive at the true top-10 threshold {float(T):.6f}")
        assert survive <= 0.02, (k, survive)
