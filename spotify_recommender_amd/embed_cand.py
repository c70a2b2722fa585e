"""EMBEDDING CANDIDATE LISTS (include/mi355rec_embed_cand.h): rank or score only the listed rows of an embedding table.
The table, the user vector, the list and the exclusion list are device tensors, a call runs on a torch stream and returns
after launching, and the answer is left in device tensors.  `rank` leaves what RestrictedEmbeddingTable.query(only=the
set of the listed ids) answers, `scores` what EmbeddingTable / HalfEmbeddingTable .scores hold at the listed rows, bit for
bit — by a gather of the listed rows, where those read the whole table (libmi355rec_embed_cand.so; a CosineEngine on a HIP
device).

Plumbing only: every value is computed by the native library.  Nothing here synchronises.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .embed import _METRICS
from .embed_stream import _NAMES, StreamedEmbeddingTable, _is_torch


class CandidateEmbeddingTable(StreamedEmbeddingTable):
    """A per-row embedding table over a CosineEngine, asked about lists of rows on streams.

    `table` is attached as StreamedEmbeddingTable attaches it: a CUDA tensor (float32, float16 or bfloat16; contiguous; on
    the engine's device; 16, 32, 64 or 128 columns) is BORROWED and a reference kept, a numpy array is copied; a node
    engine raises; nothing is converted silently.  A list holds up to 2^20 global ids in any order; an id outside the
    table's rows ranks nowhere and scores NaN with flag 0, a repeated id is ranked once and scored at every place.
    With audio_weight != 0 a call costs one audio launch over the WHOLE catalogue, however short the list is.
    The table must be closed before its engine; calls come from one host thread at a time, on any streams."""

    _load = staticmethod(capi.embed_cand_lib)
    _prefix = "mi355rec_embed_cand_"
    _what = "embedding candidate lists"

    def query(self, *a, **kw):
        raise NotImplementedError("a candidate table is asked about a list: rank(user, candidates) or scores(user, candidates)")

    def _candidates(self, candidates, device, stream):
        """The list as the library reads it: an int64 CUDA tensor [m]; a numpy array or a list is copied to the device on
        `stream` first."""
        import torch
        if not _is_torch(candidates):
            arr = np.ascontiguousarray(np.asarray(candidates, dtype=np.int64).reshape(-1))
            with torch.cuda.stream(stream):
                candidates = torch.from_numpy(arr).to(device)
        t = self._device_tensor(candidates, "candidates", torch.int64, None)
        if t.dim() != 1:
            raise ValueError(f"candidates is one list of ids, got shape {tuple(t.shape)}")
        return t

    def _request(self, user, candidates, metric, embed_weight, audio_weight, audio_row, audio, stream):
        """(the request struct without topn and exclusions, what must stay alive until the call has returned, user, list,
        the torch stream of the call)."""
        import torch
        if metric not in _METRICS:
            raise ValueError(f"metric {metric!r}: 'cosine' or 'dot'")
        user = self._device_tensor(user, "user", torch.float32, self.dim)
        if user.dim() != 1:
            raise ValueError("a candidate list is one user's: user is [dim] (user batches over a list are not served)")
        s = stream if stream is not None else torch.cuda.current_stream(user.device)
        cand = self._candidates(candidates, user.device, s)
        q = capi.EmbedCandQuery(size=ctypes.sizeof(capi.EmbedCandQuery), user_dev=user.data_ptr(),
                                candidates_dev=cand.data_ptr() if cand.numel() else None, n_candidates=int(cand.numel()), audio_row=-1, topn=0,
                                metric=_METRICS[metric], w_audio=float(audio_weight), w_embed=float(embed_weight))
        a = None
        if audio is not None:
            a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
            if a.size != capi.DIM:
                raise ValueError("an audio query is 12 floats")
            q.audio = a.ctypes.data
        elif audio_row is not None:
            q.audio_row = int(audio_row)
        return q, a, user, cand, s

    def _outputs(self, out, wanted, device, stream):
        """`out` checked against [(name, dtype, shape)], or fresh tensors handed to `stream` by the allocator."""
        import torch
        if out is not None:
            if len(out) != len(wanted):
                raise ValueError(f"out is {len(wanted)} tensors: {', '.join(name for name, _, _ in wanted)}")
            for t, (name, dtype, shape) in zip(out, wanted):
                self._device_tensor(t.reshape(-1) if t.dim() == 0 else t, f"out {name}", dtype, None)
                if tuple(t.shape) != shape and not (shape == () and t.numel() == 1):
                    raise ValueError(f"out {name} of shape {tuple(t.shape)}: {shape}")
            return tuple(out)
        with torch.cuda.stream(stream):   # (the allocator hands these to the stream that writes them)
            return tuple(torch.empty(shape, dtype=dtype, device=device) for _, dtype, shape in wanted)

    def rank(self, user, candidates, *, topn=10, metric="cosine", embed_weight=1.0, audio_weight=0.0, audio_row=None, audio=None,
             exclude=None, out=None, stream=None):
        """Enqueues the top-N over the distinct listed rows on `stream` (a torch stream; None: torch.cuda.current_stream())
        and returns without synchronising: (idx [topn] int64, -1 padded; score [topn] float32, 0 padded; count, a 0-dim
        int32) device tensors, valid in stream order.  `user`: a float32 CUDA tensor [dim].  `candidates`: an int64 CUDA
        tensor [m], m <= 2^20 (a numpy array or a list is copied to the device first).  `exclude`: None, or an int64 CUDA
        tensor [L], L <= 1024, global ids.  `audio_row` / `audio`: as StreamedEmbeddingTable.query.  `out`: (idx, score,
        count) preallocated."""
        import torch
        q, a, user, cand, s = self._request(user, candidates, metric, embed_weight, audio_weight, audio_row, audio, stream)
        n_out = max(int(topn), 0)
        idx, score, count = self._outputs(out, [("idx", torch.int64, (n_out,)), ("score", torch.float32, (n_out,)), ("count", torch.int32, ())],
                                          user.device, s)
        L = 0
        if exclude is not None:
            exclude = self._device_tensor(exclude, "exclude", torch.int64, None)
            if exclude.dim() != 1:
                raise ValueError(f"exclude of shape {tuple(exclude.shape)} for one user")
            L = int(exclude.shape[0])
        q.topn, q.n_exclude, q.exclude_dev = int(topn), L, (exclude.data_ptr() if L else None)
        res = capi.EmbedStreamResult(size=ctypes.sizeof(capi.EmbedStreamResult), out_idx_dev=idx.data_ptr(), out_score_dev=score.data_ptr(),
                                     out_count_dev=count.data_ptr())
        self._check(self._fn("enqueue_rank")(self._e, ctypes.byref(q), ctypes.byref(res), ctypes.c_void_p(s.cuda_stream)))
        del a, cand   # (the audio floats were read before the call returned; the list is the caller's, or torch's in stream order)
        return idx, score, count

    def scores(self, user, candidates, *, metric="cosine", embed_weight=1.0, audio_weight=0.0, audio_row=None, audio=None, out=None,
               stream=None):
        """Enqueues v and c of every listed row, in list order, duplicates included, and returns without synchronising:
        (v [m] float32, c [m] float32, flag [m] uint8) device tensors.  flag 1: the id is a row of the table; an id that is
        not gets NaN in v and c and flag 0.  `out`: (v, c, flag) preallocated."""
        import torch
        q, a, user, cand, s = self._request(user, candidates, metric, embed_weight, audio_weight, audio_row, audio, stream)
        m = int(cand.numel())
        v, c, flag = self._outputs(out, [("v", torch.float32, (m,)), ("c", torch.float32, (m,)), ("flag", torch.uint8, (m,))], user.device, s)
        res = capi.EmbedCandScores(size=ctypes.sizeof(capi.EmbedCandScores), out_v_dev=v.data_ptr() if m else None,
                                   out_c_dev=c.data_ptr() if m else None, out_flag_dev=flag.data_ptr() if m else None)
        self._check(self._fn("enqueue_scores")(self._e, ctypes.byref(q), ctypes.byref(res), ctypes.c_void_p(s.cuda_stream)))
        del a, cand
        return v, c, flag

    def info(self) -> dict:
        out = capi.EmbedCandInfo()
        out.size = ctypes.sizeof(capi.EmbedCandInfo)
        self._check(self._fn("info")(self._e, ctypes.byref(out)))
        d = {name: getattr(out, name) for name, _ in capi.EmbedCandInfo._fields_ if name not in ("size", "reserved")}
        d["table_dev"] = int(d["table_dev"] or 0)
        d["storage_name"] = _NAMES[d["storage"]]
        return d
