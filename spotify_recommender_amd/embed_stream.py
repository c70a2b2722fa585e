"""STREAMED EMBEDDING REQUESTS (include/mi355rec_embed_stream.h): the table, the user vectors and the exclusion lists are
device tensors, a call runs on a torch stream and returns after launching, and the answer is left in device tensors —
what EmbeddingTable / HalfEmbeddingTable / EmbeddingBatchTable answer for the same rows, bit for bit, without the round
trip through the host (libmi355rec_embed_stream.so; a CosineEngine on a HIP device).

Plumbing only: every value is computed by the native library.  Nothing here synchronises.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .embed import _METRICS, _pad, padded_dim

_NAMES = {capi.EMBED_STREAM_FP32: "fp32", capi.EMBED_HALF_FP16: "fp16", capi.EMBED_HALF_BF16: "bf16"}


def _is_torch(x) -> bool:
    return str(getattr(x, "dtype", "")).startswith("torch.")


class StreamedEmbeddingTable:
    """A per-row embedding table over a CosineEngine (one row of `table` per row of the engine), asked on streams.

    `table`: a CUDA tensor of dtype float32, float16 or bfloat16 is BORROWED — nothing is copied, a reference is kept, and
    rows rewritten with torch on a stream are what the requests enqueued behind the write on that stream see.  It must be
    contiguous, on the engine's device and 16, 32, 64 or 128 columns wide (no padded copy is made silently).  A numpy array
    (float32, or float16 attached as it is) is copied, zero-padded to a served width.
    The table must be closed before its engine; calls come from one host thread at a time, on any streams."""

    # (the library of a table and what its entry points and refusals call it: CandidateEmbeddingTable attaches its table
    # the same way to another library)
    _load = staticmethod(capi.embed_stream_lib)
    _prefix = "mi355rec_embed_stream_"
    _what = "streamed embedding requests"

    def _fn(self, name):
        return getattr(self._lib, self._prefix + name)

    def __init__(self, engine, table):
        self._e = ctypes.c_void_p()
        if getattr(engine, "_prefix", "") == "mi355rec_sharded_":
            raise ValueError(f"{self._what} are served over a CosineEngine, not a node engine")
        self._lib = self._load()
        self._engine = engine   # (kept alive: the table reads the engine's rows)
        self._table = None
        if _is_torch(table):
            import torch
            storages = {torch.float32: capi.EMBED_STREAM_FP32, torch.float16: capi.EMBED_HALF_FP16, torch.bfloat16: capi.EMBED_HALF_BF16}
            if not table.is_cuda:
                raise ValueError(f"a {table.dtype} tensor on {table.device}: a torch table is a CUDA tensor, borrowed as it is "
                                 "(pass a numpy array to have a host table copied)")
            if table.dtype not in storages:
                raise ValueError(f"a table of dtype {table.dtype}: torch.float32, torch.float16 or torch.bfloat16")
            if table.dim() != 2:
                raise ValueError("an embedding table is [rows, dim]")
            dev = table.device.index if table.device.index is not None else 0
            if dev != int(engine.device):
                raise ValueError(f"a table on cuda:{dev} for an engine on cuda:{int(engine.device)}")
            if not table.is_contiguous():
                raise ValueError("a borrowed table is contiguous (nothing is copied: call .contiguous() and keep that tensor)")
            if int(table.shape[1]) not in capi.EMBED_DIMS:
                raise ValueError(f"a borrowed table of {int(table.shape[1])} columns: 16, 32, 64 or 128 (nothing is copied: zero-pad the tensor)")
            self.storage = storages[table.dtype]
            self.user_dim = self.dim = int(table.shape[1])
            self.rows = int(table.shape[0])
            self._table = table   # (the reference that keeps the borrowed memory alive)
            rc = self._fn("create_device")(engine._h, ctypes.c_void_p(table.data_ptr()), self.rows, self.dim, self.storage,
                                                               ctypes.byref(self._e))
        else:
            half = isinstance(table, np.ndarray) and table.dtype == np.float16
            arr = np.ascontiguousarray(table) if half else np.asarray(table, dtype=np.float32)
            if arr.ndim != 2 or arr.shape[1] < 1:
                raise ValueError("an embedding table is [rows, dim]")
            self.storage = capi.EMBED_HALF_FP16 if half else capi.EMBED_STREAM_FP32
            self.user_dim = int(arr.shape[1])
            self.dim = padded_dim(self.user_dim)
            if half and self.user_dim != self.dim:   # (the word 0 is +0.0)
                padded = np.zeros((arr.shape[0], self.dim), dtype=np.float16)
                padded[:, : self.user_dim] = arr
                arr = padded
            elif not half:
                arr = _pad(arr, self.dim)
            self.rows = int(arr.shape[0])
            rc = self._fn("create")(engine._h, arr.ctypes.data_as(ctypes.c_void_p), self.rows, self.dim, self.storage,
                                                        ctypes.byref(self._e))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._fn("last_error")(None) or b"").decode("utf-8", "replace"))

    def _check(self, rc: int) -> None:
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._fn("last_error")(self._e) or b"").decode("utf-8", "replace"))

    def close(self) -> None:
        """Destroys the native table (it waits for the device); a borrowed tensor is left as it is."""
        if getattr(self, "_e", None) is not None and self._e:
            self._fn("destroy")(self._e)
            self._e = ctypes.c_void_p()
        self._engine = None
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

    def _device_tensor(self, t, what, dtype, last):
        """`t` as the library reads it: a contiguous CUDA tensor of `dtype` on the engine's device, 1 or 2 dims, `last` wide."""
        import torch
        if not _is_torch(t) or not t.is_cuda:
            raise ValueError(f"{what} is a CUDA tensor (a streamed request reads no host memory)")
        dev = t.device.index if t.device.index is not None else 0
        if dev != int(self._engine.device):
            raise ValueError(f"{what} on cuda:{dev} for a table on cuda:{int(self._engine.device)}")
        if t.dtype != dtype or t.dim() not in (1, 2) or not t.is_contiguous():
            raise ValueError(f"{what} is a contiguous {dtype} tensor of 1 or 2 dims, got {t.dtype} {tuple(t.shape)}")
        if last is not None and int(t.shape[-1]) != last:
            raise ValueError(f"{what} of {int(t.shape[-1])} columns for a table of {last}")
        return t

    def query(self, user, *, topn=10, metric="cosine", embed_weight=1.0, audio_weight=0.0, audio_row=None, audio=None, exclude=None,
              out=None, stream=None):
        """Enqueues the request on `stream` (a torch stream; None: torch.cuda.current_stream()) and returns without
        synchronising: (idx, score, count) device tensors, valid in stream order.
        `user`: a float32 CUDA tensor [dim] — one user: idx / score are [topn] (-1 / 0 padded), count a 0-dim int32 — or
        [B, dim] — a batch over an fp32 table, topn <= 128, no audio side: idx / score [B, topn], count [B].
        `exclude`: None, or an int64 CUDA tensor [L] (one user) / [B, L] (a row padded with -1), L <= 1024, global ids.
        `audio_row` (a local row) or `audio` (12 host floats, read before the call returns): the audio query of one user, needed
        when audio_weight != 0.  `out`: (idx, score, count) preallocated tensors of those shapes; else torch allocates them."""
        import torch
        if metric not in _METRICS:
            raise ValueError(f"metric {metric!r}: 'cosine' or 'dot'")
        user = self._device_tensor(user, "user", torch.float32, self.dim)
        batch = user.dim() == 2
        n_users = int(user.shape[0]) if batch else 1
        s = stream if stream is not None else torch.cuda.current_stream(user.device)
        n_out = max(int(topn), 0)
        shape = (n_users, n_out) if batch else (n_out,)
        if out is not None:
            idx, score, count = out
            for t, dtype, want, name in ((idx, torch.int64, shape, "idx"), (score, torch.float32, shape, "score"),
                                         (count, torch.int32, (n_users,) if batch else (), "count")):
                self._device_tensor(t.reshape(-1) if t.dim() == 0 else t, f"out {name}", dtype, None)
                if tuple(t.shape) != want and not (name == "count" and not batch and t.numel() == 1):
                    raise ValueError(f"out {name} of shape {tuple(t.shape)}: {want}")
        else:
            with torch.cuda.stream(s):   # (the allocator hands these to the stream that writes them)
                idx = torch.empty(shape, dtype=torch.int64, device=user.device)
                score = torch.empty(shape, dtype=torch.float32, device=user.device)
                count = torch.empty((n_users,) if batch else (), dtype=torch.int32, device=user.device)
        L = 0
        if exclude is not None:
            exclude = self._device_tensor(exclude, "exclude", torch.int64, None)
            if exclude.dim() != user.dim() or (batch and int(exclude.shape[0]) != n_users):
                raise ValueError(f"exclude of shape {tuple(exclude.shape)} for user of shape {tuple(user.shape)}")
            L = int(exclude.shape[-1])
        res = capi.EmbedStreamResult(size=ctypes.sizeof(capi.EmbedStreamResult), out_idx_dev=idx.data_ptr(), out_score_dev=score.data_ptr(),
                                     out_count_dev=count.data_ptr())
        handle = ctypes.c_void_p(s.cuda_stream)
        if batch:
            if float(audio_weight) != 0.0 or audio_row is not None or audio is not None:
                raise ValueError("a batch of users has no audio side (audio_weight must be 0)")
            q = capi.EmbedStreamUsers(size=ctypes.sizeof(capi.EmbedStreamUsers), users_dev=user.data_ptr(),
                                      exclude_dev=exclude.data_ptr() if L else None, n_users=n_users, topn=int(topn), exclude_len=L,
                                      metric=_METRICS[metric], w_embed=float(embed_weight))
            self._check(self._fn("enqueue_users")(self._e, ctypes.byref(q), ctypes.byref(res), handle))
        else:
            q = capi.EmbedStreamQuery(size=ctypes.sizeof(capi.EmbedStreamQuery), user_dev=user.data_ptr(), exclude_dev=exclude.data_ptr() if L else None,
                                      audio_row=-1, n_exclude=L, topn=int(topn), metric=_METRICS[metric], w_audio=float(audio_weight),
                                      w_embed=float(embed_weight))
            a = None
            if audio is not None:
                a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
                if a.size != capi.DIM:
                    raise ValueError("an audio query is 12 floats")
                q.audio = a.ctypes.data
            elif audio_row is not None:
                q.audio_row = int(audio_row)
            self._check(self._fn("enqueue_query")(self._e, ctypes.byref(q), ctypes.byref(res), handle))
            del a   # (read before the call returned)
        return idx, score, count

    def info(self) -> dict:
        out = capi.EmbedStreamInfo()
        out.size = ctypes.sizeof(capi.EmbedStreamInfo)
        self._check(self._fn("info")(self._e, ctypes.byref(out)))
        d = {name: getattr(out, name) for name, _ in capi.EmbedStreamInfo._fields_ if name != "size"}
        d["table_dev"] = int(d["table_dev"] or 0)
        d["storage_name"] = _NAMES[d["storage"]]
        return d
