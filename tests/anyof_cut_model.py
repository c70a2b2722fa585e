"""The numpy model of the ANY-OF pre-filter (csrc/playlist_cut.hip.h, "ANY"): per member the PLAIN cut with K = 1, through the very
functions tests/playlist_cut_model.py mirrors the device's with, as the device code calls playlist_cut_setup and playlist_cut_plain:

    AnyCut(rows, members)      playlist_cut_any_member per member: D_k of every row, |u_k|, margin_k (model(..., weights = [1])); .ok
                               is False where the kernel switches the pre-filter off for the launch (any member not claimed)
    .cuts(T)                   playlist_cut_any: q8_threshold( fl( fl(T - margin_k) / |u_k| ) ) per member
    .ruled_out(T)              playlist_cut_any_apply: a valid row is ruled out iff D_k < cut_k for EVERY member (special rows never)
"""
import numpy as np

from tests.playlist_cut_model import model
from tests.test_q8_margin import q8_codes, q8_threshold


class AnyCut:
    def __init__(self, rows, members):
        members = np.ascontiguousarray(members, np.float32).reshape(-1, 12)
        self.codes, self.valid = q8_codes(np.ascontiguousarray(rows, np.float32))
        self.per_member = [model(self.codes, self.valid, members[k:k + 1], np.ones(1, np.float32)) for k in range(members.shape[0])]
        self.ok = all(m is not None for m in self.per_member)

    def cuts(self, T):
        return [q8_threshold(np.float32(np.float32(np.float32(T) - np.float32(mm)) / np.float32(un))) for _, un, mm in self.per_member]

    def ruled_out(self, T):
        keep = ~self.valid                                   # the replica's special rows always take the chains
        for (D, _, _), cut in zip(self.per_member, self.cuts(T)):
            keep = keep | (D >= cut)
        return ~keep
