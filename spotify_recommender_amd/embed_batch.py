"""USER BATCHES over an embedding table (include/mi355rec_embed_batch.h): exact embedding top-N for many users per pass
over the table.  Every user's answer is what EmbeddingTable.query gives that user alone with audio_weight = 0, bit for
bit (libmi355rec_embed_batch.so; a handle on a HIP device).

Plumbing only: every score is computed by the native library.  With `rows=` the user vectors are the contract's in-order
float32 sums of the member rows, formed here from the host copy of the table.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .embed import _METRICS, _pad, padded_dim


class EmbeddingBatchTable:
    """A per-row embedding table over a CosineEngine (one row of `table` per row of the engine), asked for many users per
    call.  The table must be closed before its engine; one call at a time."""

    def __init__(self, engine, table, lib_path=None):
        self._lib = capi.embed_batch_lib(lib_path)
        self._e = ctypes.c_void_p()
        self._engine = engine   # (kept alive: the table reads the engine's geometry)
        arr = np.asarray(table, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] < 1:
            raise ValueError("an embedding table is float32 [rows, dim]")
        self.user_dim = int(arr.shape[1])
        self.dim = padded_dim(self.user_dim)
        self._table = _pad(arr, self.dim)   # (kept: `rows=` sums member rows on the host)
        rc = self._lib.mi355rec_embed_batch_create(engine._h, self._table.ctypes.data_as(ctypes.c_void_p), self._table.shape[0], self.dim,
                                                   ctypes.byref(self._e))
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._lib.mi355rec_embed_batch_last_error(None) or b"").decode("utf-8", "replace"))
        self.rows = int(self._table.shape[0])

    def _check(self, rc: int) -> None:
        if rc != capi.OK:
            raise capi.Mi355Error(rc, (self._lib.mi355rec_embed_batch_last_error(self._e) or b"").decode("utf-8", "replace"))

    def close(self) -> None:
        if getattr(self, "_e", None) is not None and self._e:
            self._lib.mi355rec_embed_batch_destroy(self._e)
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

    def _users_from_rows(self, rows):
        """u = e_r0, then u = fl(u + e_rk) in list order, per user (float32 numpy additions: nothing is fused)."""
        out = np.empty((len(rows), self.dim), dtype=np.float32)
        with np.errstate(all="ignore"):
            for b, members in enumerate(rows):
                members = [int(r) for r in members]
                if not 1 <= len(members) <= capi.EMBED_MAX_MEMBERS:
                    raise ValueError(f"{len(members)} member rows: 1 to {capi.EMBED_MAX_MEMBERS} are supported")
                for r in members:
                    if not 0 <= r < self.rows:
                        raise ValueError(f"Invalid song index: {r}")
                u = self._table[members[0]].copy()
                for r in members[1:]:
                    u = u + self._table[r]
                out[b] = u
        return out

    def query_users(self, *, users=None, rows=None, topn=10, metric="cosine", embed_weight=1.0, exclude=None, exclude_rows=True):
        """The top-`topn` rows of every user: (ids [B, topn] int64, -1 padded; scores [B, topn] float32, 0 padded; counts [B]).
        `users`: [B, dim] user vectors by value, or `rows`: one list of member rows (local rows) per user, summed and — unless
        exclude_rows=False — excluded from that user's results; `exclude`: None, or one sequence of global ids per user."""
        if metric not in _METRICS:
            raise ValueError(f"metric {metric!r}: 'cosine' or 'dot'")
        if (users is None) == (rows is None):
            raise ValueError("a user batch needs users by value or by rows, not both")
        if rows is not None:
            rows = [list(m) for m in rows]
            u = self._users_from_rows(rows)
        else:
            u = np.asarray(users, dtype=np.float32)
            if u.ndim != 2 or u.shape[1] not in (self.user_dim, self.dim):
                raise ValueError(f"users of shape {u.shape} for a table of {self.user_dim} columns")
            u = _pad(u, self.dim)
        n_users = int(u.shape[0])
        lists = [[] for _ in range(n_users)] if exclude is None else [list(x) for x in exclude]
        if len(lists) != n_users:
            raise ValueError(f"{len(lists)} exclusion lists for {n_users} users")
        if rows is not None and exclude_rows:
            base = int(getattr(self._engine, "row_base", 0))
            lists = [x + [r + base for r in m] for x, m in zip(lists, rows)]
        q = capi.EmbedBatchQuery()
        q.size = ctypes.sizeof(capi.EmbedBatchQuery)
        u = np.ascontiguousarray(u)
        q.users = u.ctypes.data
        q.n_users = n_users
        excl = offs = None
        if any(lists):
            offs = np.zeros(n_users + 1, dtype=np.int64)
            np.cumsum([len(x) for x in lists], out=offs[1:])
            excl = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]))
            q.exclude_global = excl.ctypes.data
            q.exclude_offsets = offs.ctypes.data
        q.topn = int(topn)
        q.metric = _METRICS[metric]
        q.w_embed = float(embed_weight)
        n_out = max(int(topn), 0)
        idx = np.empty((n_users, n_out), dtype=np.int64)
        score = np.empty((n_users, n_out), dtype=np.float32)
        count = np.zeros(n_users, dtype=np.int32)
        res = capi.EmbedBatchResult()
        res.size = ctypes.sizeof(capi.EmbedBatchResult)
        res.out_idx = idx.ctypes.data
        res.out_score = score.ctypes.data
        res.out_count = count.ctypes.data
        self._check(self._lib.mi355rec_embed_batch_query(self._e, ctypes.byref(q), ctypes.byref(res)))
        del u, excl, offs
        return idx, score, count

    def info(self) -> dict:
        out = capi.EmbedBatchInfo()
        out.size = ctypes.sizeof(capi.EmbedBatchInfo)
        self._check(self._lib.mi355rec_embed_batch_info(self._e, ctypes.byref(out)))
        return {name: getattr(out, name) for name, _ in capi.EmbedBatchInfo._fields_ if name != "size"}
