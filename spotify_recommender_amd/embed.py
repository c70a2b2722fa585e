"""EMBEDDING TABLES (include/mi355rec_embed.h): a second vector per song, learned from who listens to what, attached to an
engine; one request ranks every row by  v = audio_weight * (audio cosine) + embed_weight * (embedding similarity),
exactly, on the device (libmi355rec_embed.so; the CPU placement of a node engine is served on the host).

Plumbing only: every value is computed by the native library.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

_METRICS = {"cosine": capi.EMBED_COSINE, "dot": capi.EMBED_DOT, capi.EMBED_COSINE: capi.EMBED_COSINE, capi.EMBED_DOT: capi.EMBED_DOT}


def padded_dim(dim: int) -> int:
    """The width the library serves a table of `dim` columns at: the next of 16, 32, 64, 128 (zero columns change no sum)."""
    for d in capi.EMBED_DIMS:
        if dim <= d:
            return d
    raise ValueError(f"embedding dim {dim}: at most {capi.EMBED_DIMS[-1]} columns are supported")


def _pad(arr: np.ndarray, dim: int) -> np.ndarray:
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    if arr.shape[-1] == dim:
        return arr
    out = np.zeros(arr.shape[:-1] + (dim,), dtype=np.float32)
    out[..., : arr.shape[-1]] = arr
    return out


class EmbeddingTable:
    """A per-row embedding table over a CosineEngine or a NodeEngine (one row of `table` per row of the engine).  The table
    must be closed before its engine; one call at a time; a node engine must have no call of its own in flight."""

    _PREFIX = "mi355rec_embed_"   # (the entry points and the info struct of the library that serves this class)
    _INFO = capi.EmbedInfo

    def _fn(self, name):
        return getattr(self._lib, self._PREFIX + name)

    def __init__(self, engine, table):
        self._lib = capi.embed_lib()
        self._e = ctypes.c_void_p()
        self._engine = engine   # (kept alive: the table reads the engine's rows)
        arr = np.asarray(table, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] < 1:
            raise ValueError("an embedding table is float32 [rows, dim]")
        self.user_dim = int(arr.shape[1])
        self.dim = padded_dim(self.user_dim)
        arr = _pad(arr, self.dim)
        node = getattr(engine, "_prefix", "") == "mi355rec_sharded_"
        create = self._lib.mi355rec_embed_create_node if node else self._lib.mi355rec_embed_create
        rc = create(engine._h, arr.ctypes.data_as(ctypes.c_void_p), arr.shape[0], self.dim, ctypes.byref(self._e))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._lib.mi355rec_embed_last_error(None) or b"").decode("utf-8", "replace"))
        self.rows = int(arr.shape[0])

    def _check(self, rc: int) -> None:
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._fn("last_error")(self._e) or b"").decode("utf-8", "replace"))

    def close(self) -> None:
        if getattr(self, "_e", None) is not None and self._e:
            self._fn("destroy")(self._e)
            self._e = ctypes.c_void_p()
        self._engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _query_struct(self, user, rows, audio_row, audio, embed_weight, audio_weight, metric, exclude, topn, exclude_rows):
        """The C struct of a request and the arrays it points into (kept alive by the caller)."""
        if metric not in _METRICS:
            raise ValueError(f"metric {metric!r}: 'cosine' or 'dot'")
        q = capi.EmbedQuery()
        q.size = ctypes.sizeof(capi.EmbedQuery)
        keep = []
        if user is not None:
            u = np.asarray(user, dtype=np.float32).reshape(-1)
            if u.size != self.user_dim and u.size != self.dim:
                raise ValueError(f"user vector of {u.size} floats for a table of {self.user_dim} columns")
            u = _pad(u, self.dim)
            keep.append(u)
            q.user = u.ctypes.data
        excl = np.asarray([] if exclude is None else exclude, dtype=np.int64).reshape(-1)
        if rows is not None:
            r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
            keep.append(r)
            q.rows = r.ctypes.data
            q.k = r.size
            if exclude_rows:
                base = int(getattr(self._engine, "row_base", 0))
                excl = np.concatenate([excl, r + base])
        excl = np.ascontiguousarray(excl)
        keep.append(excl)
        q.exclude_global = excl.ctypes.data if excl.size else None
        q.n_exclude = excl.size
        q.audio_row = -1
        if audio is not None:
            a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
            if a.size != capi.DIM:
                raise ValueError("an audio query is 12 floats")
            keep.append(a)
            q.audio = a.ctypes.data
        elif audio_row is not None:
            q.audio_row = int(audio_row)
        q.topn = int(topn)
        q.metric = _METRICS[metric]
        q.w_audio = float(audio_weight)
        q.w_embed = float(embed_weight)
        return q, keep

    def query(self, *, user=None, rows=None, audio_row=None, audio=None, embed_weight=1.0, audio_weight=0.0, metric="cosine",
              exclude=None, topn=10, exclude_rows=True):
        """The top-`topn` rows by v: (ids, values) of the rows found (global ids, best first).  `user`: the user vector by
        value, or `rows`: member rows whose table rows are summed (excluded from the results unless exclude_rows=False);
        `audio_row` / `audio`: the audio query (needed when audio_weight != 0); `exclude`: further global ids."""
        q, keep = self._query_struct(user, rows, audio_row, audio, embed_weight, audio_weight, metric, exclude, topn, exclude_rows)
        n_out = max(int(topn), 0)
        idx = np.empty(n_out, dtype=np.int64)
        score = np.empty(n_out, dtype=np.float32)
        count = ctypes.c_int(0)
        res = capi.EmbedResult()
        res.size = ctypes.sizeof(capi.EmbedResult)
        res.out_idx = idx.ctypes.data
        res.out_score = score.ctypes.data
        res.out_count = ctypes.pointer(count)
        self._check(self._fn("query")(self._e, ctypes.byref(q), ctypes.byref(res)))
        del keep
        assert np.all(idx[count.value:] == -1) and np.all(score[count.value:] == 0)
        return idx[: count.value], score[: count.value]

    def scores(self, *, user=None, rows=None, audio_row=None, audio=None, embed_weight=1.0, audio_weight=0.0, metric="cosine"):
        """The parity hook: (v, c) of EVERY row, float32 arrays of `rows` entries."""
        q, keep = self._query_struct(user, rows, audio_row, audio, embed_weight, audio_weight, metric, None, 0, False)
        v = np.empty(self.rows, dtype=np.float32)
        c = np.empty(self.rows, dtype=np.float32)
        self._check(self._fn("scores")(self._e, ctypes.byref(q), v.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p)))
        del keep
        return v, c

    def info(self) -> dict:
        out = self._INFO()
        out.size = ctypes.sizeof(self._INFO)
        self._check(self._fn("info")(self._e, ctypes.byref(out)))
        return {name: getattr(out, name) for name, _ in self._INFO._fields_ if name not in ("size", "reserved")}

    def enqueue_probe(self, sink, stream=None) -> None:
        """A plain read of the table on `stream` (a torch stream or None); sink: a uint32 device tensor of >= 1024 words."""
        s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self._fn("enqueue_probe")(self._e, ctypes.c_void_p(sink.data_ptr()), s))
