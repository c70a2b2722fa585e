"""MULTI-INTEREST EMBEDDING REQUESTS (include/mi355rec_embed_multi.h): one user is K vectors — the interests a
multi-interest user model produces — and one call leaves one list: the top-N rows by their best interest, and which
interest that was.  The table, the interests and the exclusion list are device tensors, a call runs on a torch stream and
returns after launching, and the answer is left in device tensors: what K calls of StreamedEmbeddingTable.query, merged by
row, would leave, bit for bit, from one pass over the table (libmi355rec_embed_multi.so; a CosineEngine on a HIP device).

Plumbing only: every value is computed by the native library.  Nothing here synchronises.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .embed import _METRICS
from .embed_stream import _NAMES, StreamedEmbeddingTable


class MultiInterestEmbeddingTable(StreamedEmbeddingTable):
    """A per-row embedding table over a CosineEngine, asked for the best of K user vectors on streams.

    `table` is attached as StreamedEmbeddingTable attaches it: a CUDA tensor (float32, float16 or bfloat16; contiguous; on
    the engine's device; 16, 32, 64 or 128 columns) is BORROWED and a reference kept, a numpy array is copied; a node
    engine raises; nothing is converted silently.  The table must be closed before its engine; calls come from one host
    thread at a time, on any streams."""

    _load = staticmethod(capi.embed_multi_lib)
    _prefix = "mi355rec_embed_multi_"
    _what = "multi-interest embedding requests"

    def query(self, interests, *, topn=10, metric="cosine", embed_weight=1.0, audio_weight=0.0, audio_row=None, audio=None, exclude=None,
              out=None, stream=None):
        """Enqueues the request on `stream` (a torch stream; None: torch.cuda.current_stream()) and returns without
        synchronising: (idx [topn] int64, -1 padded; score [topn] float32, 0 padded; count, a 0-dim int32; interest [topn]
        int32, -1 padded) device tensors, valid in stream order.  A row's score is the largest of its values over the
        interests, its interest the lowest index that gives it.
        `interests`: a float32 CUDA tensor [K, dim], 1 <= K <= 32, or [dim] for K = 1; it is read on the stream, not copied.
        `exclude`: None, or an int64 CUDA tensor [L], L <= 1024, global ids.  `audio_row` (a local row) or `audio` (12 host
        floats, read before the call returns): the one audio query of the request, needed when audio_weight != 0.
        `out`: (idx, score, count, interest) preallocated tensors of those shapes; else torch allocates them."""
        import torch
        if metric not in _METRICS:
            raise ValueError(f"metric {metric!r}: 'cosine' or 'dot'")
        interests = self._device_tensor(interests, "interests", torch.float32, self.dim)
        K = int(interests.shape[0]) if interests.dim() == 2 else 1
        if K < 1 or K > capi.EMBED_MULTI_MAX_INTERESTS:
            raise ValueError(f"{K} interests: 1 to {capi.EMBED_MULTI_MAX_INTERESTS} (batches of multi-interest users are not served)")
        s = stream if stream is not None else torch.cuda.current_stream(interests.device)
        n_out = max(int(topn), 0)
        wanted = (("idx", torch.int64, (n_out,)), ("score", torch.float32, (n_out,)), ("count", torch.int32, ()), ("interest", torch.int32, (n_out,)))
        if out is not None:
            if len(out) != len(wanted):
                raise ValueError("out is 4 tensors: idx, score, count, interest")
            for t, (name, dtype, shape) in zip(out, wanted):
                self._device_tensor(t.reshape(-1) if t.dim() == 0 else t, f"out {name}", dtype, None)
                if tuple(t.shape) != shape and not (shape == () and t.numel() == 1):
                    raise ValueError(f"out {name} of shape {tuple(t.shape)}: {shape}")
            idx, score, count, interest = out
        else:
            with torch.cuda.stream(s):   # (the allocator hands these to the stream that writes them)
                idx, score, count, interest = (torch.empty(shape, dtype=dtype, device=interests.device) for _, dtype, shape in wanted)
        L = 0
        if exclude is not None:
            exclude = self._device_tensor(exclude, "exclude", torch.int64, None)
            if exclude.dim() != 1:
                raise ValueError(f"exclude of shape {tuple(exclude.shape)} for one user")
            L = int(exclude.shape[0])
        q = capi.EmbedMultiQuery(size=ctypes.sizeof(capi.EmbedMultiQuery), interests_dev=interests.data_ptr(), exclude_dev=exclude.data_ptr() if L else None,
                                 audio_row=-1, n_interests=K, n_exclude=L, topn=int(topn), metric=_METRICS[metric], w_audio=float(audio_weight),
                                 w_embed=float(embed_weight))
        a = None
        if audio is not None:
            a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
            if a.size != capi.DIM:
                raise ValueError("an audio query is 12 floats")
            q.audio = a.ctypes.data
        elif audio_row is not None:
            q.audio_row = int(audio_row)
        res = capi.EmbedMultiResult(size=ctypes.sizeof(capi.EmbedMultiResult), out_idx_dev=idx.data_ptr(), out_score_dev=score.data_ptr(),
                                    out_count_dev=count.data_ptr(), out_interest_dev=interest.data_ptr())
        self._check(self._fn("enqueue_query")(self._e, ctypes.byref(q), ctypes.byref(res), ctypes.c_void_p(s.cuda_stream)))
        del a   # (read before the call returned)
        return idx, score, count, interest

    def info(self) -> dict:
        out = capi.EmbedMultiInfo()
        out.size = ctypes.sizeof(capi.EmbedMultiInfo)
        self._check(self._fn("info")(self._e, ctypes.byref(out)))
        d = {name: getattr(out, name) for name, _ in capi.EmbedMultiInfo._fields_ if name not in ("size", "reserved")}
        d["table_dev"] = int(d["table_dev"] or 0)
        d["storage_name"] = _NAMES[d["storage"]]
        return d
