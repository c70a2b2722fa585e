"""RESTRICTED EMBEDDING REQUESTS (include/mi355rec_embed_sets.h): a hybrid request that leaves out a listening history of
any length (`seen`) and / or ranks only within a row set (`only`: a genre, a market, a candidate pool), exactly, over an
fp32, fp16 or bf16 table (libmi355rec_embed_sets.so).  The scan does not load a tile in which the sets admit no row.

Plumbing only: every value of a request is computed by the native library.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .embed import EmbeddingTable, _pad, padded_dim
from .embed_half import _words_of, widen


class RowSet:
    """One bit per row of a RestrictedEmbeddingTable (made by its rowset / rowset_from_mask).  Closed before its table."""

    def __init__(self, table, handle):
        self._table = table   # (kept alive: the set lives on the table's device)
        self._s = handle

    def add(self, ids) -> None:
        """Further global ids (duplicates allowed, ids outside the table's rows match nothing); seen by the next query."""
        arr = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        self._table._check(self._table._lib.mi355rec_embed_sets_rowset_add(self._s, arr.ctypes.data_as(ctypes.c_void_p), arr.size))

    @property
    def count(self) -> int:
        """The distinct rows of the table in the set."""
        return int(self._table._lib.mi355rec_embed_sets_rowset_count(self._s))

    def close(self) -> None:
        if getattr(self, "_s", None) is not None and self._s:
            self._table._lib.mi355rec_embed_sets_rowset_destroy(self._s)
            self._s = ctypes.c_void_p()
        self._table = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RestrictedEmbeddingTable(EmbeddingTable):
    """EmbeddingTable whose requests take row sets, for a CosineEngine.  `table`: a float32 table (kept as fp32, or with
    storage='fp16' / 'bf16' rounded to nearest-even on the host), or a numpy float16 array / torch float16 / bfloat16 tensor,
    attached as it is.  query takes EmbeddingTable.query's keywords and `seen` / `only`.  A node engine is not served."""

    _PREFIX = "mi355rec_embed_sets_"
    _INFO = capi.EmbedSetsInfo

    def __init__(self, engine, table, storage=None):
        self._e = ctypes.c_void_p()
        if getattr(engine, "_prefix", "") == "mi355rec_sharded_":
            raise ValueError("a restricted embedding table is served over a CosineEngine, not a node engine")
        self._lib = capi.embed_sets_lib()
        self._engine = engine   # (kept alive: the table reads the engine's rows)
        kind = str(getattr(table, "dtype", ""))
        half = storage is not None or kind in ("torch.float16", "torch.bfloat16", "float16")
        if half:
            words, self.storage = _words_of(table, storage)
        else:
            if kind.startswith("torch."):
                table = table.detach().cpu().numpy()
            words, self.storage = np.asarray(table, dtype=np.float32), capi.EMBED_SETS_FP32
        if words.ndim != 2 or words.shape[1] < 1:
            raise ValueError("an embedding table is [rows, dim]")
        self.user_dim = int(words.shape[1])
        self.dim = padded_dim(self.user_dim)
        if half and self.user_dim != self.dim:   # (the word 0 is +0.0 in both storages)
            padded = np.zeros((words.shape[0], self.dim), dtype=np.uint16)
            padded[:, : self.user_dim] = words
            words = padded
        self._stored = np.ascontiguousarray(words) if half else _pad(words, self.dim)
        ptr = self._stored.ctypes.data_as(ctypes.c_void_p)
        if half:
            rc = self._fn("create_half")(engine._h, ptr, self._stored.shape[0], self.dim, self.storage, ctypes.byref(self._e))
        else:
            rc = self._fn("create")(engine._h, ptr, self._stored.shape[0], self.dim, ctypes.byref(self._e))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._fn("last_error")(None) or b"").decode("utf-8", "replace"))
        self.rows = int(self._stored.shape[0])

    def widened(self) -> np.ndarray:
        """The float32 table the contract speaks of, [rows, dim] (dim: the served width)."""
        return self._stored if self.storage == capi.EMBED_SETS_FP32 else widen(self._stored, self.storage)

    def _new_set(self, rc, handle) -> RowSet:
        self._check(rc)
        return RowSet(self, handle)

    def rowset(self, ids) -> RowSet:
        """A row set of global ids (duplicates allowed, ids outside the table's rows match nothing)."""
        arr = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        s = ctypes.c_void_p()
        return self._new_set(self._fn("rowset_create")(self._e, arr.ctypes.data_as(ctypes.c_void_p), arr.size, ctypes.byref(s)), s)

    def rowset_from_mask(self, mask) -> RowSet:
        """A row set from one value per row of the table: non-zero (True) means in the set (labels == g, made by the caller)."""
        arr = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0).view(np.uint8)
        s = ctypes.c_void_p()
        return self._new_set(self._fn("rowset_create_mask")(self._e, arr.ctypes.data_as(ctypes.c_void_p), arr.size, ctypes.byref(s)), s)

    def query(self, *, user=None, rows=None, audio_row=None, audio=None, embed_weight=1.0, audio_weight=0.0, metric="cosine",
              exclude=None, topn=10, exclude_rows=True, seen=None, only=None):
        """EmbeddingTable.query, restricted: rows of `seen` are left out, and with `only` just its rows are ranked (RowSets
        of this table).  Member rows are added to `exclude` unless exclude_rows=False, as there."""
        q, keep = self._query_struct(user, rows, audio_row, audio, embed_weight, audio_weight, metric, exclude, topn, exclude_rows)
        ext = capi.EmbedSetsExt()
        ext.size = ctypes.sizeof(capi.EmbedSetsExt)
        ext.seen = seen._s if seen is not None else None
        ext.only = only._s if only is not None else None
        n_out = max(int(topn), 0)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        res = capi.EmbedResult()
        res.size = ctypes.sizeof(capi.EmbedResult)
        res.out_idx = idx.ctypes.data
        res.out_score = score.ctypes.data
        res.out_count = ctypes.pointer(count)
        self._check(self._fn("query")(self._e, ctypes.byref(q), ctypes.byref(ext), ctypes.byref(res)))
        del keep
        assert np.all(idx[count.value:] == -1) and np.all(score[count.value:] == 0)
        return idx[: count.value], score[: count.value]

    def scores(self, **kw):
        raise NotImplementedError("the parity hook is EmbeddingTable's and HalfEmbeddingTable's, over the same arithmetic")

    def enqueue_probe(self, sink, stream=None):
        raise NotImplementedError("the probe is EmbeddingTable's and HalfEmbeddingTable's")
