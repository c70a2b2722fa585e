"""The numpy mirror of the count launch's two cuts (csrc/playlist_cut.hip.h, "BOUNDED" and "PLAIN"), float32 arithmetic, operation for
operation, built on tests/playlist_cut_model.py's functions:

    BoundedCut(rows, members)       playlist_cut_setup, kind plain, for the unweighted call: D, |u|, margin_mean (playlist_cut_model.model
                                    with every weight 1); .ok False where the kernel switches the pre-filter off for the launch
    .cuts(b)                        (cut_d, cut_hi) at the floor's score b: the launch's threshold key is floor_thr = (image(b) << 32) - 1,
                                    so playlist_cut_refresh sees the float just BELOW b (the image (thr >> 32)) and playlist_cut_plain
                                    gives cut_d; playlist_cut_proven sees b itself (the image (thr + 1) >> 32) and gives cut_hi
    .ruled_out(b), .proven_in(b)    the valid rows with D < cut_d, with D >= cut_hi; the others take the chains
"""
import numpy as np

from tests.bounded_oracle import image
from tests.playlist_cut_model import model
from tests.test_q8_margin import DOT_SCALE, q8_codes, q8_threshold

F32 = np.float32
NEVER = 2 ** 31 - 1                                             # kPlCutNever


def score_below(b):
    """ordered_to_score(image(b) - 1): the float just below b in the keys' order (-0.0 and +0.0 are one)."""
    o = np.uint32(image(F32(b)) - np.uint32(1))
    u = (o & np.uint32(0x7fffffff)) if (o & np.uint32(0x80000000)) else ~o
    return np.array([u], np.uint32).view(F32)[0]


def cut_proven(t, margin_mean, un):
    """playlist_cut_proven: a valid row with D >= this matches the floor's score t."""
    with np.errstate(all="ignore"):
        q = F32(F32(F32(t) + F32(margin_mean)) / F32(un))
    if not (q < F32(2)):
        return NEVER
    return int(np.ceil(F32(max(q, F32(-2)) * DOT_SCALE))) + 1


class BoundedCut:
    def __init__(self, rows, members):
        codes, self.valid = q8_codes(np.ascontiguousarray(rows, F32))
        members = np.ascontiguousarray(members, F32).reshape(-1, 12)
        m = model(codes, self.valid, members, np.ones(len(members), F32))
        self.ok = m is not None
        if self.ok:
            self.D, self.un, self.mm = m

    def cuts(self, b):
        with np.errstate(all="ignore"):
            cut_d = q8_threshold(F32(F32(score_below(b) - F32(self.mm)) / self.un))
        return cut_d, cut_proven(b, self.mm, self.un)

    def ruled_out(self, b):
        return self.valid & (self.D < self.cuts(b)[0])

    def proven_in(self, b):
        return self.valid & (self.D >= self.cuts(b)[1])
