"""HALF-PRECISION EMBEDDING TABLES (include/mi355rec_embed_half.h): an fp16 or bf16 table is attached to an engine as it
is — the device holds and reads the 2 bytes per value the model produced — and every answer is that of EmbeddingTable over
the widened table, bit for bit (libmi355rec_embed_half.so).

Plumbing only: every value of a request is computed by the native library.  What this module computes on the host is the
storage itself: to_storage (round an fp32 table to nearest-even words) and widen (the exact fp32 values of words).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .embed import EmbeddingTable, padded_dim

_STORAGES = {"fp16": capi.EMBED_HALF_FP16, "bf16": capi.EMBED_HALF_BF16, capi.EMBED_HALF_FP16: capi.EMBED_HALF_FP16,
             capi.EMBED_HALF_BF16: capi.EMBED_HALF_BF16}
_NAMES = {capi.EMBED_HALF_FP16: "fp16", capi.EMBED_HALF_BF16: "bf16"}


def _storage(storage) -> int:
    if storage not in _STORAGES:
        raise ValueError(f"storage {storage!r}: 'fp16' or 'bf16'")
    return _STORAGES[storage]


def to_storage(table, storage) -> np.ndarray:
    """The uint16 words of a float32 array rounded to nearest-even in `storage` ('fp16' / 'bf16').  A NaN stays a NaN; a
    value beyond the storage's largest finite one becomes inf (fp16: from 65520 on)."""
    code = _storage(storage)
    arr = np.ascontiguousarray(table, dtype=np.float32)
    if code == capi.EMBED_HALF_FP16:
        with np.errstate(over="ignore"):
            return arr.astype(np.float16).view(np.uint16)
    bits = arr.view(np.uint32).astype(np.uint64)
    words = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(arr)
    if nan.any():   # (the carry of the rounding may turn a NaN's payload into inf or 0: keep sign and exponent, set the quiet bit)
        words[nan] = ((bits[nan] >> 16) | 0x40).astype(np.uint16)
    return words


def widen(words, storage) -> np.ndarray:
    """W(x): the exact float32 value of every uint16 word of `storage`."""
    code = _storage(storage)
    w = np.ascontiguousarray(words, dtype=np.uint16)
    if code == capi.EMBED_HALF_FP16:
        return w.view(np.float16).astype(np.float32)
    return (w.astype(np.uint32) << 16).view(np.float32)


def _words_of(table, storage):
    """(uint16 words [rows, dim], storage code) of what a caller hands to HalfEmbeddingTable."""
    kind = str(getattr(table, "dtype", ""))
    given = None
    if kind in ("torch.float16", "torch.bfloat16"):   # (a torch tensor: its words as they are)
        import torch
        given = capi.EMBED_HALF_FP16 if kind == "torch.float16" else capi.EMBED_HALF_BF16
        words = table.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    elif isinstance(table, np.ndarray) and table.dtype == np.float16:
        given = capi.EMBED_HALF_FP16
        words = np.ascontiguousarray(table).view(np.uint16)
    if given is not None:
        if storage is not None and _storage(storage) != given:
            raise ValueError(f"a {_NAMES[given]} table with storage={storage!r}")
        return words, given
    if storage is None:
        raise ValueError("a float32 table needs storage='fp16' or 'bf16' (it is rounded to nearest-even on the host)")
    if kind.startswith("torch."):
        table = table.detach().cpu().numpy()
    return to_storage(np.asarray(table, dtype=np.float32), storage), _storage(storage)


class HalfEmbeddingTable(EmbeddingTable):
    """EmbeddingTable over 16-bit storage, for a CosineEngine.  `table`: a numpy float16 array or a torch float16 / bfloat16
    tensor, attached as it is (its storage is inferred), or a float32 table with storage='fp16' / 'bf16', rounded to
    nearest-even on the host.  query / scores / info / enqueue_probe are EmbeddingTable's, keyword for keyword; user vectors
    stay float32.  A node engine is not served: attach EmbeddingTable(engine, half.widened()) there — the same bits."""

    _PREFIX = "mi355rec_embed_half_"
    _INFO = capi.EmbedHalfInfo

    def __init__(self, engine, table, storage=None):
        self._e = ctypes.c_void_p()
        if getattr(engine, "_prefix", "") == "mi355rec_sharded_":
            raise ValueError("a half-precision table is served over a CosineEngine, not a node engine: "
                             "EmbeddingTable(engine, table.widened()) answers the same bits there")
        self._lib = capi.embed_half_lib()
        self._engine = engine   # (kept alive: the table reads the engine's rows)
        words, self.storage = _words_of(table, storage)
        if words.ndim != 2 or words.shape[1] < 1:
            raise ValueError("an embedding table is [rows, dim]")
        self.user_dim = int(words.shape[1])
        self.dim = padded_dim(self.user_dim)
        if self.user_dim != self.dim:   # (the word 0 is +0.0 in both storages)
            padded = np.zeros((words.shape[0], self.dim), dtype=np.uint16)
            padded[:, : self.user_dim] = words
            words = padded
        self._words = np.ascontiguousarray(words)
        rc = self._fn("create")(engine._h, self._words.ctypes.data_as(ctypes.c_void_p), self._words.shape[0], self.dim, self.storage,
                                ctypes.byref(self._e))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._fn("last_error")(None) or b"").decode("utf-8", "replace"))
        self.rows = int(self._words.shape[0])

    def words(self) -> np.ndarray:
        """The table as the device holds it: uint16 [rows, dim] (dim: the served width)."""
        return self._words

    def widened(self) -> np.ndarray:
        """The float32 table the contract speaks of: W of every stored word, [rows, dim]."""
        return widen(self._words, self.storage)
