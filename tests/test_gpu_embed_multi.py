"""MULTI-INTEREST EMBEDDING REQUESTS on the GPU (include/mi355rec_embed_multi.h, csrc/embed_multi.hip.h): what
MultiInterestEmbeddingTable leaves in device tensors — ids, order, score bits, count, padding and the interest of every
result — bit for bit, after one stream.synchronize(), against
  identity 1: StreamedEmbeddingTable.query on the same engine, for K = 1;
  identity 2: the merge of K StreamedEmbeddingTable.query answers (tests/embed_multi_cases.merge), for every K;
  the numpy oracle (tests/embed_multi_cases.expected: embed_cases.expected's v per interest, the maximum over the finite
  ones, the lowest argmax, embed_oracle.topn), with out_interest its argmax and out_score the matched interest's v bits.
Every storage and dim; K in {1, 2, P - 1, P, P + 1, 2P + 1, 32} with P read from info; both metrics, both signs of
w_embed, the audio side by row and by value, topn 1 / 10 / 257 / 1024 / rows + 1, 0 / 1 / 1024 hostile exclusions; row
counts 1, t - 1, t, t + 1, 2t + 1 and grid * t + 1; a row base; two streams; the steady state of the candidate list; and the
pointed cases a multi-interest scan can get wrong.  Hostile means values, never addresses."""
import functools

import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_half_cases as hc
from tests import embed_multi_cases as mc
from tests import embed_oracle as eo
from tests import embed_steady_cases as ssc

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = [16, 32, 64, 128]
STORAGES = ["f32", "fp16", "bf16"]


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _table_tensor(table, storage):
    """(the device tensor a model would hold, the fp32 table the contract speaks of)."""
    import torch
    from spotify_recommender_amd.embed_half import to_storage, widen
    if storage == "f32":
        return _dev(table), table
    words = to_storage(table, storage)
    return _dev(words.view(np.int16)).view(torch.float16 if storage == "fp16" else torch.bfloat16), widen(words, storage)


def _open(feats, table, storage="f32", **kw):
    """(engine, the multi-interest table and the streamed table over ONE borrowed tensor, the fp32 rows)."""
    from spotify_recommender_amd import CosineEngine, MultiInterestEmbeddingTable
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    eng = CosineEngine(feats, **kw)
    t, wide = _table_tensor(table, storage)
    return eng, MultiInterestEmbeddingTable(eng, t), StreamedEmbeddingTable(eng, t), wide


@functools.lru_cache(maxsize=None)
def _geometry(d, storage):
    """(tile rows, chunk width P, the grid of a table with at least that many tiles), asked of the library."""
    from spotify_recommender_amd import CosineEngine, MultiInterestEmbeddingTable
    t, _ = _table_tensor(np.ones((1, d), F32), storage)
    with CosineEngine(np.ones((1, 12), F32)) as eng, MultiInterestEmbeddingTable(eng, t) as mt:
        info = mt.info()
        grid = ssc.grid_of(eng.stats().compute_units)
    assert info["tile_rows"] == 2048 // (d // (4 if storage == "f32" else 8)) and info["max_interests"] == 32 and info["query_launches"] == 3
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "spotify_recommender_amd" / "csrc" / "embed_multi.hip.h").read_text()
    assert info["pass_interests"] == int(re.search(r"#define MI355REC_EMBED_MULTI_PASS (\d+)", src).group(1)) and info["pass_users"] == 1
    return info["tile_rows"], info["pass_interests"], grid


def _kw(req):
    return {k: v for k, v in req.items() if k not in ("exclude",)}


def _ask(mt, us, req, stream=None):
    """One multi-interest request; (idx, score, count, interest) on the host after one synchronise."""
    import torch
    excl = _dev(np.asarray(req["exclude"], np.int64)) if req.get("exclude") else None
    idx, sc, cnt, who = mt.query(_dev(np.asarray(us, F32)), exclude=excl, stream=stream, **_kw(req))
    (stream or torch.cuda.current_stream()).synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item()), who.cpu().numpy()


def _ask_single(st, u, req):
    import torch
    excl = _dev(np.asarray(req["exclude"], np.int64)) if req.get("exclude") else None
    idx, sc, cnt = st.query(_dev(np.asarray(u, F32)), exclude=excl, **_kw(req))
    torch.cuda.current_stream().synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())


def _same(got, want, topn, what):
    """got = (idx, score, count, interest) [topn]; want = (ids, scores, interests) of the results alone."""
    idx, sc, cnt, who = got
    wi, ws, wk = want
    assert cnt == wi.size, f"{what}: count {cnt}, want {wi.size}"
    assert idx[:cnt].tolist() == wi.tolist(), f"{what}: ids differ (got {idx[:8].tolist()}, want {wi[:8].tolist()})"
    assert np.array_equal(eo.bits(sc[:cnt]), eo.bits(ws)), f"{what}: score bits differ"
    assert who[:cnt].tolist() == np.asarray(wk).tolist(), f"{what}: interests differ (got {who[:8].tolist()}, want {np.asarray(wk)[:8].tolist()})"
    assert idx.shape == (topn,) and sc.shape == (topn,) and who.shape == (topn,)
    assert np.all(idx[cnt:] == -1) and np.all(eo.bits(sc[cnt:]) == 0) and np.all(who[cnt:] == -1), f"{what}: padding"


def _check(mt, st, feats, wide, us, req, what, row_base=0, identities=True, topn=eo.topn, ranked=True):
    """One request against the oracle and, with `identities`, against the streamed library on the same engine."""
    us = np.asarray(us, F32).reshape(-1, wide.shape[1])
    got = _ask(mt, us, req)
    ids, sc, ks, vs = mc.expected(feats, wide, us, req, row_base, topn, ranked)
    _same(got, (ids, sc, ks), req["topn"], f"{what} vs the oracle")
    matched = vs[ks, ids - row_base] + F32(0)
    assert np.array_equal(eo.bits(got[1][: ids.size]), eo.bits(matched)), f"{what}: a score is not its interest's v"
    if identities:
        singles = []
        for u in us:
            i1, s1, c1 = _ask_single(st, u, req)
            singles.append((i1[:c1], s1[:c1]))
        _same(got, mc.merge(singles, req["topn"]), req["topn"], f"{what} vs the merge of {len(us)} streamed answers (identity 2)")
        if len(us) == 1:
            i1, s1, c1 = _ask_single(st, us[0], req)
            assert got[2] == c1 and np.array_equal(got[0], i1) and np.array_equal(eo.bits(got[1]), eo.bits(s1)), f"{what}: identity 1"
            assert np.all(got[3][:c1] == 0)
    return got


def _request(i, n, row_base=0):
    """Request i of a cycle in which every metric, sign, audio side, topn and exclusion length meets the others."""
    metric = ("cosine", "dot")[i % 2]
    w = (1.0, -0.5, 2.0)[i % 3]
    topn = (1, 10, 257, 1024, min(n + 1, 1024))[i % 5]
    req = dict(metric=metric, embed_weight=w, topn=topn)
    audio = i % 4
    if audio == 1:
        req.update(audio_weight=1.0, audio_row=(7 * i) % n)
    elif audio == 3:
        req.update(audio_weight=-1.5, audio=np.random.default_rng(i).random(12, dtype=F32))
    L = (0, 1, 1024)[(i // 2) % 3]
    if L:
        req["exclude"] = mc.hostile_exclusions(n, L, row_base, seed=i)
    return req


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("d", DIMS)
def test_every_row_count_and_every_k(d, storage):
    t, P, _ = _geometry(d, storage)
    Ks = mc.interest_counts(P)
    assert len(Ks) % 5 != 4, "request i + len(Ks) + 1 must not repeat request i's topn: K and topn would never cross"
    i = 0
    for n in (1, t - 1, t, t + 1, 2 * t + 1):
        feats, table = hc.float_catalogue(n, d)
        eng, mt, st, wide = _open(feats, table, storage)
        with eng, mt, st:
            before = mt.info()
            asked = audio = excluding = 0
            for K in Ks:
                req = _request(i, n)
                _check(mt, st, feats, wide, mc.interests(K, d, seed=i), req, f"{storage} n={n} d={d} K={K} request {i}")
                asked, audio, excluding, i = asked + 1, audio + ("audio_weight" in req), excluding + ("exclude" in req), i + 1
            i += 1   # (one more per row count: K meets another topn, metric, weight and list at every row count)
            after = mt.info()
            assert after["enqueues"] - before["enqueues"] == asked and after["scores_launches"] == audio
            assert after["launches"] - before["launches"] == 3 * asked + audio + excluding


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("d", DIMS)
def test_a_second_round_of_one_row(d, storage):
    """grid * t + 1 rows: every workgroup scans a full tile and workgroup 0 a second one that holds a single row."""
    t, P, grid = _geometry(d, storage)
    n = grid * t + 1
    rng = np.random.default_rng(d)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    us = mc.interests(P + 1, d, seed=5)
    table[n - 1] = us[P] * F32(3.0)   # the last row is the best row of the last interest
    eng, mt, st, wide = _open(feats, table, storage)
    with eng, mt, st:
        assert mt.info()["grid"] == grid
        req = dict(metric="cosine", embed_weight=1.0, topn=10, audio_weight=0.25, audio_row=n - 1)
        got = _check(mt, st, feats, wide, us, req, f"{storage} n={n} d={d}", identities=False, topn=ssc.topn, ranked=False)
        assert n - 1 in got[0].tolist()
        req = dict(metric="dot", embed_weight=1.0, topn=1024, exclude=mc.hostile_exclusions(n, 1024))
        _check(mt, st, feats, wide, us[:2], req, f"{storage} n={n} d={d} dot", topn=ssc.topn, ranked=False)


@pytest.mark.parametrize("storage,d", [("fp16", 16), ("f32", 16)])
def test_the_steady_state_of_the_candidate_list(storage, d):
    """V ascends with the row index, so along every workgroup's stride every tile appends a full tile of candidates and the
    list is compacted again and again, its threshold handed from tile to tile; top-128 and top-1024 over one table.  The
    table is as small as the shipped grid allows for that: a workgroup scans tiles b, b + grid, ..., and the list-occupancy
    model of tests/embed_steady_cases.py (the same trigger and capacity: it reads them from embed.hip.h, and
    embed_multi.hip.h states them in the same words) says how many rounds two mid-loop compactions take."""
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "spotify_recommender_amd" / "csrc" / "embed_multi.hip.h").read_text()
    assert re.search(r"int compact_at = 2 \* a\.topk > 256 \? 2 \* a\.topk : 256;\s*if \(compact_at > kCandLimit\) compact_at = kCandLimit;", src)
    assert "constexpr int kCandCap = kCandLimit + kMaxTileRows;" in src and "if (c >= compact_at)" in src
    t, P, grid = _geometry(d, storage)
    layout = ssc.Layout(storage, d)
    assert layout.tile_rows == t
    rounds = max(ssc.min_rounds(layout, topk) for topk in (128, 1024))
    n = ssc.sizes(t, grid, rounds)
    rng = np.random.default_rng(11 * d)
    table = rng.standard_normal((n, d), dtype=F32)
    from spotify_recommender_amd.embed_half import to_storage, widen
    wide = table if storage == "f32" else widen(to_storage(table, storage), storage)
    us = mc.interests(P + 1, d, seed=9)
    feats = np.ones((n, 12), F32)
    base = dict(metric="dot", embed_weight=1.0)
    V, k = mc.best(mc.per_interest(feats, wide, us, base, ranked=False))
    order = np.argsort(V, kind="stable")
    table, V, k = np.ascontiguousarray(table[order]), V[order], k[order]   # (v_k is a function of the row alone: they go with it)
    del wide
    eng, mt, st, _ = _open(feats, table, storage)
    with eng, mt, st:
        assert mt.info()["grid"] == grid and -(-n // t) >= rounds * grid
        assert np.all(np.diff(V) >= 0)
        for topk in (128, 1024):
            _, compactions, _ = ssc.peaks(layout, V, grid, topk)
            assert compactions >= 2
            ids, sc = ssc.topn(V, topk)
            got = _ask(mt, us, dict(base, topn=topk))
            _same(got, (ids, sc, k[ids]), topk, f"rising {storage} d={d} top-{topk}")
            assert got[0].min() >= n - 2 * topk - 1, "the answer of a rising table is its end"


def test_a_shard_with_a_row_base_and_two_streams():
    """Ids and exclusions are global; 12 enqueues alternate over two streams with no ordering by the caller."""
    import torch
    n, d, base = 1500, 32, 1_000_000
    feats, table = ec.catalogue(n, d)
    eng, mt, st, wide = _open(feats, table, "f32", row_base=base)
    with eng, mt, st:
        for i, K in enumerate((1, 3, 32)):
            req = dict(metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=3, topn=40,
                       exclude=[[], [base + 7, 7, base + n, base + n - 1, base, -1, base + 7], [base + r for r in range(1024)]][i])
            got = _check(mt, st, feats, wide, mc.interests(K, d, seed=i), req, f"row_base K={K}", row_base=base)
            assert got[2] and got[0][: got[2]].min() >= base and not set(got[0].tolist()) & set(req["exclude"])
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        sets = [_dev(mc.interests(1 + i % 5, d, seed=20 + i)) for i in range(12)]
        torch.cuda.synchronize()
        outs = []
        for i, us in enumerate(sets):
            req = dict(metric="dot" if i % 3 else "cosine", embed_weight=1.0, topn=100)
            if i % 4 == 0:
                req.update(audio_weight=1.0, audio_row=i)
            outs.append((req, mt.query(us, stream=streams[i % 2], **req)))
        for s in streams:
            s.synchronize()
        for i, (req, (idx, sc, cnt, who)) in enumerate(outs):
            ids, wsc, ks, _ = mc.expected(feats, wide, sets[i].cpu().numpy(), req, base)
            _same((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item()), who.cpu().numpy()), (ids, wsc, ks), 100, f"enqueue {i}")


# ---- the pointed cases ----

@pytest.mark.parametrize("storage,d", [("f32", 16), ("fp16", 64), ("bf16", 128)])
def test_a_padded_slot_never_wins(storage, d):
    """Positive rows, negative interests: every cosine is < 0.  At K = P + 1 the last chunk is short; a padded zero slot would
    score c = 0 and win every row."""
    t, P, _ = _geometry(d, storage)
    n = 2 * t + 1
    rng = np.random.default_rng(d)
    table = rng.random((n, d), dtype=F32) + F32(0.25)
    us = -(rng.random((P + 1, d), dtype=F32) + F32(0.25))
    feats = rng.random((n, 12), dtype=F32)
    eng, mt, st, wide = _open(feats, table, storage)
    with eng, mt, st:
        for metric in ("cosine", "dot"):
            got = _check(mt, st, feats, wide, us, dict(metric=metric, embed_weight=1.0, topn=50), f"padded slots {storage} d={d} {metric}")
            assert got[2] == 50 and np.all(got[1] < 0), "a zero slot took part in the maximum"


def test_equal_values_report_the_lower_interest():
    n, d = 700, 32
    feats, table = ec.catalogue(n, d)
    eng, mt, st, wide = _open(feats, table)
    with eng, mt, st:
        u = mc.interests(1, d)[0]
        other = mc.interests(1, d, seed=3)[0]
        got = _check(mt, st, feats, wide, np.stack([other, u, u, other]), dict(metric="cosine", embed_weight=1.0, topn=100), "two identical interests")
        assert set(got[3][: got[2]].tolist()) <= {0, 1}, "interest 2 repeats 1 and 3 repeats 0: neither is ever the lowest argmax"


def test_a_zero_norm_interest_beside_real_ones():
    """The zero vector scores c = 0 for every row under cosine: it wins exactly the rows every other interest dislikes."""
    n, d = 900, 16
    feats, table = ec.catalogue(n, d)
    eng, mt, st, wide = _open(feats, table, "fp16")
    with eng, mt, st:
        us = mc.interests(3, d, seed=1)
        us[2] = 0
        got = _check(mt, st, feats, wide, us, dict(metric="cosine", embed_weight=1.0, topn=1024), "a zero interest")
        assert 2 in got[3][: got[2]].tolist() and np.all(got[1][: got[2]] >= 0)
        _check(mt, st, feats, wide, us, dict(metric="cosine", embed_weight=-1.0, topn=1024), "a zero interest, negative weight")
        _check(mt, st, feats, wide, np.zeros((2, d), F32), dict(metric="cosine", embed_weight=1.0, topn=10), "only zero interests")


def test_rows_that_are_not_finite():
    """A row with a NaN forms no key; a row whose dot overflows against one interest forms a key only from a finite v_k."""
    n, d = 600, 16
    rng = np.random.default_rng(4)
    table = rng.standard_normal((n, d), dtype=F32)
    table[10, 3] = np.nan
    table[11] = F32(1e30)
    feats = rng.random((n, 12), dtype=F32)
    us = rng.standard_normal((3, d), dtype=F32)
    us[0] = F32(1e30)            # tree(row 11, interest 0) overflows to +inf: not a value
    us[1, :] = 0
    us[1, 0] = F32(1e-3)         # finite against row 11
    eng, mt, st, wide = _open(feats, table)
    with eng, mt, st:
        _check(mt, st, feats, wide, us, dict(metric="cosine", embed_weight=1.0, topn=n), "non-finite rows, cosine")   # (a NaN norm: c = 0)
        got = _check(mt, st, feats, wide, us, dict(metric="dot", embed_weight=1.0, topn=n), "non-finite rows, dot")
        found = got[0][: got[2]].tolist()
        assert 10 not in found and got[2] == n - 1
        assert got[3][found.index(11)] != 0
        vs = mc.per_interest(feats, wide, us, dict(metric="dot", embed_weight=1.0))
        assert not np.isfinite(vs[0, 11]) and np.isfinite(vs[1, 11]) and not np.isfinite(vs[:, 10]).any()
        got = _ask(mt, us[:1], dict(metric="dot", embed_weight=1.0, topn=n))
        assert 11 not in got[0].tolist(), "the only v of the row is infinite"


def test_minus_zero_and_plus_zero_tie():
    """Under dot, interest 0 gives the rows of one half-space -0.0 and interest 1 gives them +0.0: equal by the float
    comparison, so interest 0 holds them, and the score is reported as +0.0."""
    n, d = 300, 16
    rng = np.random.default_rng(6)
    table = np.zeros((n, d), F32)
    table[:, 0] = np.abs(rng.standard_normal(n).astype(F32)) + F32(0.5)
    us = np.zeros((3, d), F32)
    us[0] = F32(-0.0)      # rows >= 0 against the all -0.0 vector: every product is -0.0, so the tree sums to -0.0 ...
    us[1] = F32(0.0)       # ... and to +0.0 against the all +0.0 vector
    us[2, 0] = F32(-1.0)   # a real, negative interest
    feats = rng.random((n, 12), dtype=F32)
    eng, mt, st, wide = _open(feats, table)
    with eng, mt, st:
        vs = mc.per_interest(feats, wide, us, dict(metric="dot", embed_weight=1.0))
        assert np.all(eo.bits(vs[0]) == 0x80000000) and np.all(eo.bits(vs[1]) == 0)
        got = _check(mt, st, feats, wide, us, dict(metric="dot", embed_weight=1.0, topn=20), "-0.0 beside +0.0")
        assert np.all(got[3] == 0) and np.all(eo.bits(got[1]) == 0)
        got = _check(mt, st, feats, wide, us[[1, 0, 2]], dict(metric="dot", embed_weight=1.0, topn=20), "+0.0 beside -0.0")
        assert np.all(got[3] == 0) and np.all(eo.bits(got[1]) == 0)


@pytest.mark.parametrize("storage,d", [("f32", 128), ("bf16", 16)])
def test_a_key_from_the_last_chunk_and_from_the_first(storage, d):
    """K = 32: the best interest at k = 31, then at k = 0 — the running maximum is carried through every chunk."""
    t, P, _ = _geometry(d, storage)
    n = t + 1
    rng = np.random.default_rng(d + 1)
    table = rng.random((n, d), dtype=F32) + F32(0.25)
    feats = rng.random((n, 12), dtype=F32)
    weak = -(rng.random((32, d), dtype=F32) + F32(0.25))
    strong = rng.random(d, dtype=F32) + F32(0.25)
    eng, mt, st, wide = _open(feats, table, storage)
    with eng, mt, st:
        for at in (31, 0):
            us = weak.copy()
            us[at] = strong
            got = _check(mt, st, feats, wide, us, dict(metric="cosine", embed_weight=1.0, topn=64), f"{storage} d={d} best at {at}")
            assert np.all(got[3] == at) and np.all(got[1] > 0)


def test_refusals_launch_nothing():
    import ctypes

    import torch
    from spotify_recommender_amd import capi
    n, d = 40, 16
    feats, table = ec.catalogue(n, d)
    eng, mt, st, wide = _open(feats, table)
    with eng, mt, st:
        us = _dev(mc.interests(3, d))
        before = mt.info()
        for kw, text in ((dict(topn=0), r"topn 0 out of \[1, 1024\]"), (dict(topn=1025), r"topn 1025 out of \[1, 1024\]"),
                         (dict(embed_weight=0.0), "embed_weight 0"), (dict(audio_weight=4.5, audio_row=1), "audio_weight 4.5"),
                         (dict(audio_weight=1.0), "got row -1"), (dict(audio_weight=1.0, audio_row=n), "got row 40"),
                         (dict(exclude=_dev(np.zeros(1025, np.int64))), r"n_exclude 1025 out of \[0, 1024\]")):
            with pytest.raises(capi.Mi355Error, match=text) as err:
                mt.query(us, **kw)
            assert err.value.code == capi.ERR_INVALID_ARG
        for bad, text in ((_dev(np.zeros((33, d), F32)), "33 interests"), (_dev(np.zeros((0, d), F32)), "0 interests"),
                          (np.zeros((2, d), F32), "interests is a CUDA tensor"), (_dev(np.zeros((2, d + 1), F32)), "interests of 17 columns")):
            with pytest.raises(ValueError, match=text):
                mt.query(bad)
        L = capi.embed_multi_lib()
        out = torch.empty(5, dtype=torch.int64, device="cuda:0")
        res = capi.EmbedMultiResult(size=40, out_idx_dev=out.data_ptr())
        for field, value, text in (("size", 70, b"embed multi query of size 70"), ("flags", 1, b"flags 0x1"), ("reserved", 3, b"reserved 0x3"),
                                   ("n_interests", 0, b"n_interests 0 out of [1, 32]"), ("n_interests", 33, b"n_interests 33 out of [1, 32]"),
                                   ("interests_dev", us.data_ptr() + 4, b"interests_dev is not 16-byte aligned"), ("interests_dev", None, b"null interests_dev"),
                                   ("metric", 2, b"metric 2")):
            q = capi.EmbedMultiQuery(size=72, interests_dev=us.data_ptr(), n_interests=3, audio_row=-1, topn=5, w_embed=1.0)
            setattr(q, field, value)
            assert L.mi355rec_embed_multi_enqueue_query(mt._e, ctypes.byref(q), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
            assert text in L.mi355rec_embed_multi_last_error(mt._e), text
        q = capi.EmbedMultiQuery(size=72, interests_dev=us.data_ptr(), n_interests=3, audio_row=-1, topn=5, w_embed=1.0)
        assert L.mi355rec_embed_multi_enqueue_query(mt._e, ctypes.byref(q), ctypes.byref(capi.EmbedMultiResult(size=40)), None) == capi.ERR_INVALID_ARG
        assert b"null out_idx_dev" in L.mi355rec_embed_multi_last_error(mt._e)
        after = mt.info()
        assert (after["launches"], after["enqueues"]) == (before["launches"], before["enqueues"]), "a refused call launches nothing"
        # out_score, out_count and out_interest are optional (a result that ends at out_idx_dev), and the table still answers
        q = capi.EmbedMultiQuery(size=64, interests_dev=us.data_ptr(), n_interests=3, audio_row=-1, topn=5, w_embed=1.0)   # (ends at w_embed)
        res = capi.EmbedMultiResult(size=16, out_idx_dev=out.data_ptr())
        assert L.mi355rec_embed_multi_enqueue_query(mt._e, ctypes.byref(q), ctypes.byref(res), None) == capi.OK
        torch.cuda.synchronize()
        ids, _, _, _ = mc.expected(feats, wide, us.cpu().numpy(), dict(metric="cosine", embed_weight=1.0, topn=5))
        assert out.cpu().tolist() == ids.tolist()
