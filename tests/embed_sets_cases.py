"""Tables, row sets and the expected answers of the RESTRICTED EMBEDDING REQUEST tests (include/mi355rec_embed_sets.h).
Catalogues and requests are tests/embed_cases.py's and tests/embed_half_cases.py's; the reference stays
tests/embed_oracle.py, unchanged: v of every row from eo.values over the (widened) table, then
eo.topn(v, topn, exclude = the request's exclusions + the ids of `seen` + the complement of `only`)."""
import numpy as np

from tests import embed_cases as ec
from tests import embed_half_cases as hc
from tests import embed_oracle as eo

F32 = np.float32
STORAGES = ["f32", "fp16", "bf16"]
DIMS = [16, 32, 64, 128]


def tile_rows(d, storage):
    """Rows of one 32 KiB tile: 4 (fp32) or 8 (half) stored values per 16-byte load, 2048 loads."""
    return 2048 // (d // (4 if storage == "f32" else 8))


def given(n, d, storage, seed=0):
    """(feats, what a caller hands to RestrictedEmbeddingTable): ec.catalogue's fp32 table, or hc.catalogue's words as a
    float16 array / bfloat16 tensor.  The hostile rows of both are values: NaN, inf, 1e19, subnormals, 65520, 3e38."""
    if storage == "f32":
        return ec.catalogue(n, d, seed)
    feats, words = hc.catalogue(n, d, storage, seed)
    return feats, hc.as_given(words, storage)


def row_sets(n, seed=0):
    """{name: sorted local rows} at n rows: empty, every row, one bit at row 0 and at row n - 1, rows 31 and 32 alone (the
    word edge; what of it the table has), every other row, a random 1 % and a random half."""
    rng = np.random.default_rng(31 * n + seed)
    rows = np.arange(n, dtype=np.int64)
    return {
        "empty": rows[:0],
        "all": rows,
        "first": rows[:1],
        "last": rows[n - 1:],
        "edge": rows[31:33],
        "alternate": rows[::2],
        "percent": np.sort(rng.choice(n, max(1, n // 100), replace=False)).astype(np.int64),
        "half": np.sort(rng.choice(n, max(1, n // 2), replace=False)).astype(np.int64),
    }


def values(feats, table, req):
    """v of every row of a request (ec.expected's, without a selection): computed once and shared by every set."""
    metric = eo.DOT if req["metric"] == "dot" else eo.COSINE
    u = np.asarray(req["user"], F32) if "user" in req else eo.user_from_rows(table, req["rows"])
    audio = req.get("audio")
    if audio is None and "audio_row" in req:
        audio = feats[req["audio_row"]]
    v, _ = eo.values(table, u, metric, req["embed_weight"], req.get("audio_weight", 0.0), feats, audio)
    v.setflags(write=False)
    return v


def expected(v, req, seen=None, only=None, row_base=0):
    """(ids, scores) by the oracle; seen / only: local rows or None."""
    n = v.size
    excl = [int(x) for x in req.get("exclude", [])] + [int(r) + row_base for r in req.get("rows", [])]
    if seen is not None:
        excl += (np.asarray(seen, np.int64) + row_base).tolist()
    if only is not None:
        excl += (np.setdiff1d(np.arange(n, dtype=np.int64), np.asarray(only, np.int64)) + row_base).tolist()
    return eo.topn(v, req["topn"], excl, row_base)


def answers_nothing(n, seen, only):
    """What the host bitmaps show: only is empty, seen holds every row, or only is a subset of seen."""
    if only is not None and len(only) == 0:
        return True
    if seen is not None and len(np.unique(seen)) == n:
        return True
    return seen is not None and only is not None and np.isin(only, seen).all()


def check(tab, v, req, what, seen=None, only=None, seen_set=None, only_set=None, row_base=0):
    """One restricted query against the oracle, bit for bit; returns the ids."""
    ids, sc = expected(v, req, seen, only, row_base)
    gi, gs = tab.query(**req, seen=seen_set, only=only_set)
    assert gi.tolist() == ids.tolist(), f"{what}: ids differ (got {gi[:8].tolist()}, want {ids[:8].tolist()}, counts {gi.size} / {ids.size})"
    assert np.array_equal(eo.bits(gs), eo.bits(sc)), f"{what}: score bits differ"
    return gi
