"""The numpy models of the playlist pre-filter, one mirror per device function of csrc/playlist_cut.hip.h (and of the prologue of
csrc/playlist.hip.h that feeds it): float32 arithmetic, operation for operation.  The five margin tests (test_playlist_margin,
test_weighted_margin, test_prior_margin, test_distance_margin, test_scaled_margin) import from here and from nowhere else, so which
numpy function stands for which device function is written in one place:

    fp32_norm, seq_sqnorm, norm          query_norm / playlist_sqnorm (core.hip.h, playlist.hip.h): the sequential fp32 sum of squares
    stored_norms                         q8_build_kernel's second output (replica_q8.hip.h): the side values of a distance request
    mean_direction, weighted_direction   playlist_prologue: u and |u| (all weights 1: the unweighted kernel's u bit for bit)
    unweighted_model, model              playlist_cut_setup, kind plain: D, |u| and margin_mean (cut: playlist_cut_plain =
                                         q8_threshold((T - margin_mean) / |u|), tests/test_q8_margin.py)
    ruled_out                            playlist_cut_setup + playlist_cut_prior_base + playlist_cut_prior + playlist_cut_int
    DistanceCut                          playlist_cut_setup, kind distance; .ruled_out: playlist_cut_distance_base +
                                         playlist_cut_distance + playlist_cut_int
    ScaledCut                            playlist_cut_scaled_query + playlist_cut_setup, kind scaled; .ruled_out: scaled_code_norm +
                                         playlist_cut_scaled_base + playlist_cut_scaled + playlist_cut_int
"""
import numpy as np

from tests.test_q8_margin import DOT_SCALE, S, q8_codes, q8_digits
from tests.weighted_oracle import weight_sum

F32 = np.float32
ULP = np.float32(2.0 ** -24)                                  # kPlUlp
CLAMP = np.float32(2.0 ** 30)                                 # kPlCutClamp
MIN_NORM, MAX_NORM = np.float32(1.005e-4), np.float32(1e18)   # kBqMinNorm, kBqMaxNorm
PRIOR_ULPS = np.float32(96.0)                                 # kPlPriorUlps
A_MIN, A_MAX = F32(2.0 ** -10), F32(8.0)                      # kPlScaleMinMax, kPlScaleMaxMax
FLOOR = F32(2.0 ** -6)                                        # kPlScaleFloor
STEP = F32(F32(1.001) / F32(254.0))                           # kPlScaleStep


def fp32_norm(v):
    s = np.float32(0)
    for x in np.asarray(v, np.float32):
        s = np.float32(s + np.float32(x * x))
    return np.float32(np.sqrt(s))


def seq_sqnorm(v):
    """Sequential fp32 sum of squares over the last axis (multiply, round, add, round)."""
    v = np.asarray(v, np.float32)
    acc = np.zeros(v.shape[:-1], np.float32)
    with np.errstate(all="ignore"):
        for j in range(v.shape[-1]):
            acc = (acc + (v[..., j] * v[..., j]).astype(np.float32)).astype(np.float32)
    return acc


def stored_norms(feats):
    """q8_build_kernel's second output."""
    with np.errstate(all="ignore"):
        return np.sqrt(seq_sqnorm(feats)).astype(np.float32)


def norm(v):
    with np.errstate(all="ignore"):
        return np.sqrt(seq_sqnorm(v)).astype(F32)


def mean_direction(members):
    """(u, |u|, ok) as the kernel computes them; ok: the bound may be claimed for this playlist."""
    members = np.asarray(members, np.float32)
    qn = [fp32_norm(q) for q in members]
    ok = all(np.float32(1.005e-4) <= n <= np.float32(1e18) for n in qn)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (members[0] / qn[0]).astype(np.float32)
        for q, n in zip(members[1:], qn[1:]):
            u = (u + (q / n).astype(np.float32)).astype(np.float32)
        u = (u / np.float32(len(members))).astype(np.float32)
    un = fp32_norm(u)
    return u, un, bool(ok and np.isfinite(un) and un >= np.float32(1e-3))


def weighted_direction(members, weights):
    """(u, |u|, ok) as the kernel computes them; ok: the bound may be claimed for this playlist."""
    members = np.asarray(members, np.float32)
    w = np.asarray(weights, np.float32)
    W = weight_sum(w)
    qn = [fp32_norm(q) for q in members]
    ok = all(np.float32(1.005e-4) <= n <= np.float32(1e18) for n in qn)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (w[0] * (members[0] / qn[0]).astype(np.float32)).astype(np.float32)
        for q, n, wk in zip(members[1:], qn[1:], w[1:]):
            u = (u + (wk * (q / n).astype(np.float32)).astype(np.float32)).astype(np.float32)
        u = (u / W).astype(np.float32)
    un = fp32_norm(u)
    return u, un, bool(ok and np.isfinite(un) and un >= np.float32(1e-3))


def unweighted_model(rows, members):
    """(D, valid, |u|, margin_mean) or None where the kernel turns the pre-filter off: the unweighted kernel's own margin, (2K + 32) ulp,
    K ulp tighter than the (3K + 32) of `model` below, which the kernel uses for every call now."""
    u, un, ok = mean_direction(members)
    if not ok:
        return None
    k, valid = q8_codes(rows)
    Q, h, l, qok = q8_digits(u)
    if not qok:
        return None
    D = k @ Q
    M = np.float32(np.abs(Q).sum()) * np.float32(1 / 254.0 / 32000) * np.float32(1 + 1e-5) + np.float32(3.4642 * 0.5 / 32000) + np.float32(3e-5)
    mm = np.float32(un * M + np.float32(4e-6) + np.float32(2 * len(members) + 32) * ULP)
    return D, valid, un, float(mm)


def model(codes, valid, members, weights):
    """(D, |u|, margin_mean), or None where the kernel turns the pre-filter off."""
    u, un, ok = weighted_direction(members, weights)
    if not ok:
        return None
    Q, h, l, qok = q8_digits(u)
    if not qok:
        return None
    D = codes @ Q
    M = np.float32(np.abs(Q).sum()) * np.float32(1 / 254.0 / 32000) * np.float32(1 + 1e-5) + np.float32(3.4642 * 0.5 / 32000) + np.float32(3e-5)
    mm = np.float32(un * M + np.float32(4e-6) + np.float32(3 * len(members) + 32) * ULP)
    return D, un, float(mm)


def ruled_out(D, valid, un, margin_mean, T, beta, priors):
    """The rows the kernel's per-row cut rules out at threshold T (float32 arithmetic, operation for operation)."""
    un = np.float32(un)
    mp = np.float32(np.float32(margin_mean) + PRIOR_ULPS * ULP)
    with np.errstate(over="ignore"):
        base = np.float32(np.float32(np.float32(np.float32(T) - mp) / un) * DOT_SCALE)
        bs = np.float32(np.float32(np.float32(beta) * DOT_SCALE) / un)
        c = (base - (np.asarray(priors, np.float32) * bs).astype(np.float32)).astype(np.float32)
    cut = np.trunc(np.clip(c, -CLAMP, CLAMP)).astype(np.int64) - 1
    return valid & (D < cut)


class DistanceCut:
    """The launch's constants, or ok == False where the kernel switches the pre-filter off for the launch."""

    def __init__(self, codes, members):
        q = np.ascontiguousarray(members, np.float32).reshape(-1, 12)
        k = q.shape[0]
        with np.errstate(all="ignore"):
            q2k = seq_sqnorm(q)
            qn = np.sqrt(q2k).astype(np.float32)
            c = q[0].copy()
            for m in range(1, k):
                c = (c + q[m]).astype(np.float32)
            c = (c / np.float32(k)).astype(np.float32)
            cn = np.float32(np.sqrt(seq_sqnorm(c)))
            self.ok = bool(np.all((qn >= MIN_NORM) & (qn <= MAX_NORM)) and MIN_NORM <= cn <= MAX_NORM)
            if not self.ok:
                return
            chat = (c * (np.float32(1) / cn)).astype(np.float32)                         # q8_query: q[j] * inv * S
            Q = np.clip(np.rint((chat * np.float32(S)).astype(np.float32)), -S, S).astype(np.int64)
            self.D = codes @ Q
            margin = np.float32(np.float32(np.abs(Q).sum()) * np.float32(np.float32(1.0 / 254.0) / np.float32(S)) * np.float32(1 + 1e-5)
                                + np.float32(3.4642 * 0.5 / S) + np.float32(3e-5))
            q2 = q2k[0]
            for m in range(1, k):
                q2 = np.float32(q2 + q2k[m])
            eps = np.float32(np.float32(4 * k + 128) * ULP)
            self.q2e = np.float32(np.float32(q2 / np.float32(k)) * np.float32(np.float32(1) - eps))
            self.s2c = np.float32(DOT_SCALE / np.float32(np.float32(2) * cn))
            self.c0 = np.float32(DOT_SCALE * np.float32(margin + eps))
            self.a1 = np.float32(self.s2c * np.float32(np.float32(1) - eps))
            self.ok = bool(np.isfinite(np.float32(self.q2e * self.s2c)))
            self.cn, self.margin = cn, margin

    def ruled_out(self, valid, s, T, rcp_ulps=0):
        with np.errstate(all="ignore"):
            b = np.float32(np.float32(self.q2e - np.float32(T)) * self.s2c)
            r = (np.float32(1) / s).astype(np.float32)
            for _ in range(abs(rcp_ulps)):
                r = np.nextafter(r, np.float32(np.inf if rcp_ulps > 0 else -np.inf))
            c = (((self.a1 * s).astype(np.float32) + (b * r).astype(np.float32)).astype(np.float32) - self.c0).astype(np.float32)
            c = np.where(np.isnan(c), -CLAMP, np.clip(c, -CLAMP, CLAMP))                  # (fmaxf / fminf drop a NaN)
            cut = np.trunc(c).astype(np.int64) - 1
            claimed = (s >= MIN_NORM) & (s <= MAX_NORM)
            return valid & claimed & (self.D < cut)


class ScaledCut:
    """The launch's constants, or ok == False where the kernel switches the pre-filter off for the launch."""

    def __init__(self, codes, members, weights, a):
        a = np.asarray(a, F32)
        q = (np.ascontiguousarray(members, F32).reshape(-1, 12) * a).astype(F32)
        k = q.shape[0]
        w = np.ones(k, F32) if weights is None else np.asarray(weights, F32)
        wsum = F32(k) if weights is None else weight_sum(w)
        self.ok = False
        with np.errstate(all="ignore"):
            qn = norm(q)
            if not np.all((qn >= MIN_NORM) & (qn <= MAX_NORM)):
                return
            u = (w[0] * (q[0] / qn[0]).astype(F32)).astype(F32)
            for m in range(1, k):
                u = (u + (w[m] * (q[m] / qn[m]).astype(F32)).astype(F32)).astype(F32)
            u = (u / wsum).astype(F32)
            a_max = a.max()
            self.ab = (a / a_max).astype(F32)
            uq = (self.ab * u).astype(F32)
            bn = F32(norm(uq))
            self.e = F32(F32(norm(self.ab) * STEP) + F32(8.0) * ULP)
            den_floor = F32(F32(2e-4) / F32(a_max * qn.min()))
            l_floor = max(FLOOR, den_floor)
            self.gk_min = F32(F32(l_floor + self.e) * F32(F32(1) + F32(64) * ULP))
            if not (den_floor <= F32(0.5) and A_MIN <= a_max <= A_MAX):
                return
            if not (MIN_NORM <= bn <= MAX_NORM and bn >= F32(1e-3)):
                return
            inv = F32(F32(1) / bn)
            Q = np.clip(np.rint(((uq * inv).astype(F32) * F32(S)).astype(F32)), -S, S).astype(np.int64)
            self.D = codes @ Q
            self.margin = F32(F32(np.abs(Q).sum()) * F32(F32(1.0 / 254.0) / F32(S)) * F32(1 + 1e-5) + F32(3.4642 * 0.5 / S) + F32(3e-5))
            self.margin_scaled = F32(F32(4e-6) + F32(F32(3 * k) + F32(64)) * ULP)
            self.c0 = F32(DOT_SCALE * F32(self.margin + F32(16) * ULP))
            self.bn = bn
            acc = np.zeros(codes.shape[0], F32)
            for j in range(12):
                p = (self.ab[j] * codes[:, j].astype(F32)).astype(F32)
                acc = (acc + (p * p).astype(F32)).astype(F32)
            self.root = np.sqrt(acc).astype(F32)
            self.ok = True

    def ruled_out(self, valid, T, sqrt_ulps=0):
        with np.errstate(all="ignore"):
            root = self.root
            for _ in range(abs(sqrt_ulps)):
                root = np.nextafter(root, F32(np.inf if sqrt_ulps > 0 else -np.inf))
            gk = (root * F32(F32(1) / F32(127))).astype(F32)
            tm = F32(F32(T) - self.margin_scaled)
            base = F32(F32(tm / self.bn) * DOT_SCALE)
            fmul = F32(F32(1) - F32(16) * ULP) if tm >= 0 else F32(F32(1) + F32(16) * ULP)
            fadd = -self.e if tm >= 0 else self.e
            f = ((gk * fmul).astype(F32) + fadd).astype(F32)
            c = ((base * f).astype(F32) - self.c0).astype(F32)
            c = np.where(np.isnan(c), -CLAMP, np.clip(c, -CLAMP, CLAMP))
            cut = np.trunc(c).astype(np.int64) - 1
            return valid & (gk >= self.gk_min) & (self.D < cut)
