"""A numpy mirror of the MANHATTAN pre-filter (csrc/playlist_cut.hip.h, "MANHATTAN": playlist_cut_l1_apply and the constants
anyof_prologue and anyof_cut_refresh store), operation for operation, rows vectorised:

    eps = (13 K + 64) 2^-24;   ce = fl(1 - eps);   ke1 = fl( (float)K fl(fl(12 * 1.001) / 254) );   kt = fl( (float)K T )
    sc  = fl(s fl(1 / 127)),  s the row's stored norm;     xt_j = fl( (float)b_j sc ),  b_j the row's replica byte
    acc = the fp32 sum, in the order g = 0..2, k = 0..K-1, j = 4g..4g+3, of | fl(q_kj - xt_j) |
    ruled out  iff  the row is claimed  and  fl(acc ce) > fl( fl(s ke1) + kt )
    claimed: not special (a valid replica row) and s in [1.005e-4, 1e18];   the launch has the cut only where every member's
    norm (sqrtf of the sequential sum of squares) is <= 1e18 (false for NaN)."""
import numpy as np

from tests.playlist_cut_model import norm

F32 = np.float32
ULP = F32(2.0 ** -24)
MIN_NORM, MAX_NORM = F32(1.005e-4), F32(1e18)
HALF_STEPS = F32(F32(F32(12.0) * F32(1.001)) / F32(254.0))   # kL1HalfSteps


class ManhattanCut:
    def __init__(self, codes, members):
        self.codes = np.asarray(codes, np.int64)
        self.q = np.ascontiguousarray(members, F32).reshape(-1, 12)
        self.k = self.q.shape[0]
        with np.errstate(all="ignore"):
            self.ok = bool(np.all(norm(self.q) <= MAX_NORM))                     # (false for NaN)
        self.ce = F32(F32(1.0) - F32(F32(13 * self.k + 64) * ULP))
        self.ke1 = F32(F32(self.k) * HALF_STEPS)

    def lower_sum(self, s):
        """acc of every row: float32 [n]."""
        s = np.asarray(s, F32)
        with np.errstate(all="ignore"):
            sc = (s * F32(F32(1.0) / F32(127.0))).astype(F32)
            acc = np.zeros(s.shape[0], F32)
            for g in range(3):
                xt = (self.codes[:, 4 * g:4 * g + 4].astype(F32) * sc[:, None]).astype(F32)
                for m in range(self.k):
                    for jj in range(4):
                        t = (self.q[m, 4 * g + jj] - xt[:, jj]).astype(F32)
                        acc = (acc + np.abs(t)).astype(F32)
        return acc

    def ruled_out(self, valid, s, T, acc=None):
        """The rows the kernel rules out at the threshold T (as m)."""
        s = np.asarray(s, F32)
        acc = self.lower_sum(s) if acc is None else acc
        with np.errstate(all="ignore"):
            kt = F32(F32(self.k) * F32(T))
            claimed = np.asarray(valid, bool) & (s >= MIN_NORM) & (s <= MAX_NORM)
            lhs = (acc * self.ce).astype(F32)
            rhs = ((s * self.ke1).astype(F32) + kt).astype(F32)
            return claimed & (lhs > rhs)
