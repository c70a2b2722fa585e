"""Catalogues for the HALF-PRECISION EMBEDDING TABLE tests (include/mi355rec_embed_half.h): tests/embed_cases.py's
catalogue narrowed to 16-bit words, with the rows that only half storage makes hostile.  Requests and the check are
tests/embed_cases.py's, unchanged: the reference of every test is the fp32 contract over the WIDENED table."""
import numpy as np

from tests import embed_cases as ec

F32 = np.float32
STORAGES = ["fp16", "bf16"]
# 65504: the largest finite fp16; 65520: the first value that rounds to inf there; 2^-24: the smallest fp16 subnormal
# (a kernel that flushes subnormals scores the row as zero); 3e38: finite in bf16, inf in fp16
HALF_ROWS = {12: F32(65504.0), 13: F32(65520.0), 14: F32(2.0 ** -24), 15: F32(3e38)}


def float_catalogue(n, d, seed=0):
    """(feats, fp32 table): ec.catalogue and, from 17 rows on, the four half-specific rows in rows 12 to 15."""
    feats, table = ec.catalogue(n, d, seed)
    if n >= 17:
        for row, value in HALF_ROWS.items():
            table[row] = value
    return feats, table


def catalogue(n, d, storage, seed=0):
    """(feats, uint16 words [n, d]) of float_catalogue rounded to `storage`."""
    from spotify_recommender_amd.embed_half import to_storage
    feats, table = float_catalogue(n, d, seed)
    return feats, to_storage(table, storage)


def as_given(words, storage):
    """The words as a caller holds a half table: a numpy float16 array, or a torch bfloat16 tensor."""
    if storage == "fp16":
        return words.view(np.float16)
    import torch
    return torch.from_numpy(words.view(np.int16).copy()).view(torch.bfloat16)
