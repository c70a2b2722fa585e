"""Catalogues, tables and requests for the EMBEDDING TABLE tests (CPU placement and GPU alike), and the one check both
use: every request's (v, c) of every row and its top-N against tests/embed_oracle.py, bit for bit."""
import numpy as np

from tests import embed_oracle as eo

F32 = np.float32


def catalogue(n, d, seed=0):
    """(feats [n, 12], table [n, d]): random rows, exact duplicates (ties that the row index breaks) and, from 17 rows on,
    hostile table rows: zero, 1e19 entries whose squares overflow, NaN, inf, subnormals."""
    rng = np.random.default_rng(1000 * d + n + seed)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    if n >= 5:
        feats[3], table[3] = feats[1], table[1]
        feats[n - 1], table[n - 1] = feats[1], table[1]
    if n >= 17:
        table[5] = 0
        table[6] = F32(1e19)
        table[7, 2] = np.nan
        table[8, d - 1] = np.inf
        table[9] = F32(1e-40)
        table[10] = -table[1]
        table[11, :4] = F32(-1e19)
    return feats, table


def requests(n, d, seed=0):
    """Request kwargs for EmbeddingTable.query (scores takes them without topn / exclude): u by value and from K = 1, 3, 32
    rows, both metrics, w_audio == 0, negative weights, topn 1 / 257 / 1024 / > n, exclusions with duplicates and foreign ids,
    hostile user vectors."""
    rng = np.random.default_rng(77 * d + n + seed)
    user = rng.standard_normal(d, dtype=F32)
    pick = lambda k: [int(x) for x in rng.integers(0, n, k)]
    huge = user.copy()
    huge[: d // 2] = F32(1e19)
    tiny = np.full(d, 1e-30, F32)
    reqs = [
        dict(user=user, metric="cosine", embed_weight=1.0, topn=10),
        dict(rows=pick(3), metric="cosine", embed_weight=0.25, audio_weight=1.0, audio_row=n // 2, topn=257,
             exclude=[0, 0, n - 1, n + 5, 2 ** 31 + 7, n // 2]),
        dict(rows=pick(32), metric="dot", embed_weight=-0.5, audio_weight=-1.5, audio=rng.random(12, dtype=F32), topn=1024),
        dict(rows=pick(1), metric="dot", embed_weight=2.0, topn=1),
        dict(user=np.zeros(d, F32), metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=min(1, n - 1), topn=min(n + 5, 1024)),
        dict(user=huge, metric="cosine", embed_weight=-1.0, topn=10),
        dict(user=tiny, metric="cosine", embed_weight=1.0, audio_weight=0.5, audio=np.zeros(12, F32), topn=10),
        dict(user=huge, metric="dot", embed_weight=4.0, audio_weight=-4.0, audio_row=0, topn=10, exclude=list(range(0, min(n, 1024)))),
    ]
    return reqs


def expected(feats, table, req, row_base=0):
    """(v, c, ids, scores) of a request by the oracle; rows of `req` are LOCAL to table."""
    metric = eo.DOT if req["metric"] == "dot" else eo.COSINE
    u = np.asarray(req["user"], F32) if "user" in req else eo.user_from_rows(table, req["rows"])
    audio = req.get("audio")
    if audio is None and "audio_row" in req:
        audio = feats[req["audio_row"]]
    v, c = eo.values(table, u, metric, req["embed_weight"], req.get("audio_weight", 0.0), feats, audio)
    excl = list(req.get("exclude", [])) + [r + row_base for r in req.get("rows", [])]
    ids, sc = eo.topn(v, req["topn"], excl, row_base)
    return v, c, ids, sc


def same_floats(got, want):
    """Bit for bit; a NaN matches any NaN."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(eo.bits(got)[~nan], eo.bits(want)[~nan])


def check(tab, feats, table, req, what, row_base=0, scores=True):
    v, c, ids, sc = expected(feats, table, req, row_base)
    if scores:
        kw = {k: val for k, val in req.items() if k not in ("topn", "exclude")}
        gv, gc = tab.scores(**kw)
        assert same_floats(gc, c), f"{what}: c differs in {int(np.sum(eo.bits(gc) != eo.bits(c)))} rows"
        assert same_floats(gv, v), f"{what}: v differs in {int(np.sum(eo.bits(gv) != eo.bits(v)))} rows"
    gi, gs = tab.query(**req)
    assert gi.tolist() == ids.tolist(), f"{what}: ids differ (got {gi[:8].tolist()}, want {ids[:8].tolist()}, counts {gi.size} / {ids.size})"
    assert np.array_equal(eo.bits(gs), eo.bits(sc)), f"{what}: score bits differ"
