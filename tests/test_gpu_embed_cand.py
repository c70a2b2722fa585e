"""EMBEDDING CANDIDATE LISTS on the GPU (include/mi355rec_embed_cand.h, csrc/embed_cand.hip.h): what
CandidateEmbeddingTable leaves in device tensors, bit for bit after one stream.synchronize().  rank: ids, order, score
bits, count and padding against RestrictedEmbeddingTable.query(only=rowset(the same ids)) on the same engine and against
tests/embed_oracle.py's topn over the listed rows (half storage: over the widened table).  scores: v, c and the flag
against EmbeddingTable / HalfEmbeddingTable .scores indexed by the list, NaN and flag 0 for ids outside the table.  The
sizes are those at which the gather can go wrong: every list length around one tile `t` (taken from info), a list that
gives every workgroup of the widest grid a tile and one entry more, 2^20 entries; the lists are ascending, reversed, random
with repeats, one row throughout, hostile ids mixed in, no id inside the table; a row base; streams.  Hostile means values,
never addresses.

Leave-out budget: 0 cases.  Every storage expresses every value used (a half table is compared over its widened words)."""
import ctypes

import numpy as np
import pytest

from tests import embed_batch_cases as bc
from tests import embed_cases as ec
from tests import embed_half_cases as hc
from tests import embed_oracle as eo

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = [16, 32, 64, 128]
STORAGES = ["f32", "fp16", "bf16"]
QUIET_NAN = 0x7FC00000


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _table_tensor(table, storage):
    """(the device tensor a model would hold, the fp32 table the contract speaks of, what the synchronous libraries take)."""
    import torch
    from spotify_recommender_amd.embed_half import to_storage, widen
    if storage == "f32":
        return _dev(table), table, table
    words = to_storage(table, storage)
    t = _dev(words.view(np.int16)).view(torch.float16 if storage == "fp16" else torch.bfloat16)
    return t, widen(words, storage), hc.as_given(words, storage)


class _Opened:
    """One engine with the candidate table over a borrowed tensor and the synchronous tables over the same rows."""

    def __init__(self, feats, table, storage="f32", **kw):
        from spotify_recommender_amd import CosineEngine
        from spotify_recommender_amd.embed import EmbeddingTable
        from spotify_recommender_amd.embed_cand import CandidateEmbeddingTable
        from spotify_recommender_amd.embed_half import HalfEmbeddingTable
        from spotify_recommender_amd.embed_sets import RestrictedEmbeddingTable
        self.feats, self.storage, self.row_base = feats, storage, kw.get("row_base", 0)
        self.eng = CosineEngine(feats, **kw)
        self.tensor, self.wide, given = _table_tensor(table, storage)
        self.ct = CandidateEmbeddingTable(self.eng, self.tensor)
        self.only = RestrictedEmbeddingTable(self.eng, given)
        self.sync = EmbeddingTable(self.eng, given) if storage == "f32" else HalfEmbeddingTable(self.eng, given)
        self.n = int(table.shape[0])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for x in (self.ct, self.only, self.sync, self.eng):
            x.close()


def _requests(n, d, seed=0):
    """topn 1, 10, 1024 and one above the listed rows; both metrics; exclusions of 0, 1 and 1024 ids (in the list and not);
    the audio side by row and by value."""
    rng = np.random.default_rng(91 * d + n + seed)
    user = rng.standard_normal(d, dtype=F32)
    return [
        dict(user=user, metric="cosine", embed_weight=1.0, topn=10),
        dict(user=user, metric="dot", embed_weight=-0.5, topn=1024, exclude=[int(x) for x in rng.integers(-3, n + 4, 1024)]),
        dict(user=user, metric="cosine", embed_weight=0.25, audio_weight=1.0, audio_row=n // 2, topn=1, exclude=[n // 3]),
        dict(user=rng.standard_normal(d, dtype=F32), metric="dot", embed_weight=2.0, audio_weight=-1.5, audio=rng.random(12, dtype=F32), topn=257),
    ]


def _lists(n, m, rng, row_base=0):
    """{name: m global ids}: the contents the gather must take."""
    hostile = np.array([-1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, row_base - 1, row_base + n, row_base + n + 9, 2 ** 31 + 1, 2 ** 40],
                       np.int64)
    lists = {
        "ascending": row_base + np.arange(m, dtype=np.int64) % n,
        "reversed": row_base + (n - 1 - np.arange(m, dtype=np.int64) % n),
        "random": row_base + rng.integers(0, n, m),
        "one row": np.full(m, row_base + n - 1, np.int64),
        "outside": np.resize(hostile, m),
    }
    mixed = lists["random"].copy()
    at = rng.random(m) < 0.3
    mixed[at] = np.resize(hostile, int(at.sum()))
    lists["hostile"] = mixed
    return lists


def _values(o, req):
    """(v, c) of every row by the oracle over the widened table: computed once per request and shared."""
    v, c, _, _ = ec.expected(o.feats, o.wide, dict(req, topn=1, exclude=[]))
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def _listed(o, ids):
    """The distinct local rows a list names."""
    local = np.asarray(ids, np.int64)
    inside = (local >= o.row_base) & (local < o.row_base + o.n) & (local >= 0)
    return np.unique(local[inside] - o.row_base)


def _oracle_rank(o, v, ids, req):
    """embed_oracle.topn over the listed rows: every other row forms no key."""
    only = np.full(o.n, np.nan, F32)
    rows = _listed(o, ids)
    only[rows] = v[rows]
    return eo.topn(only, req["topn"], req.get("exclude", []), o.row_base)


def _rank(o, ids, req, stream=None, out=None):
    import torch
    kw = {k: val for k, val in req.items() if k not in ("user", "exclude")}
    excl = _dev(np.asarray(req["exclude"], np.int64)) if req.get("exclude") else None
    idx, sc, cnt = o.ct.rank(_dev(np.asarray(req["user"], F32)), _dev(np.asarray(ids, np.int64)), exclude=excl, stream=stream, out=out, **kw)
    (stream or torch.cuda.current_stream()).synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())


def _same(got, want, topn, what):
    idx, sc, cnt = got
    wi, ws = want
    assert cnt == wi.size, f"{what}: count {cnt}, want {wi.size}"
    assert idx[:cnt].tolist() == wi.tolist(), f"{what}: ids differ (got {idx[:8].tolist()}, want {wi[:8].tolist()})"
    assert np.array_equal(eo.bits(sc[:cnt]), eo.bits(ws)), f"{what}: score bits differ"
    assert idx.shape == (topn,) and np.all(idx[cnt:] == -1) and np.all(eo.bits(sc[cnt:]) == 0), f"{what}: padding"


def _check_rank(o, v, ids, req, what, only_set=True):
    got = _rank(o, ids, req)
    want = _oracle_rank(o, v, ids, req)
    _same(got, want, req["topn"], f"{what} against the oracle")
    if only_set:
        ids = np.asarray(ids, np.int64)
        with o.only.rowset(ids[ids >= 0]) as rs:   # (a row set refuses a negative id, which in a list matches nothing)
            _same(got, o.only.query(**req, only=rs), req["topn"], f"{what} against the ONLY set")
    assert not set(got[0][: got[2]].tolist()) & set(req.get("exclude", []))
    return got


def _check_scores(o, all_v, all_c, ids, req, what):
    import torch
    kw = {k: val for k, val in req.items() if k not in ("user", "exclude", "topn")}
    v, c, flag = o.ct.scores(_dev(np.asarray(req["user"], F32)), _dev(np.asarray(ids, np.int64)), **kw)
    torch.cuda.current_stream().synchronize()
    v, c, flag = v.cpu().numpy(), c.cpu().numpy(), flag.cpu().numpy()
    ids = np.asarray(ids, np.int64)
    inside = (ids >= o.row_base) & (ids < o.row_base + o.n) & (ids >= 0)
    assert flag.dtype == np.uint8 and np.array_equal(flag, inside.astype(np.uint8)), f"{what}: flags"
    assert np.all(eo.bits(v[~inside]) == QUIET_NAN) and np.all(eo.bits(c[~inside]) == QUIET_NAN), f"{what}: an id outside the table is the quiet NaN"
    rows = ids[inside] - o.row_base
    assert np.array_equal(eo.bits(v[inside]), eo.bits(all_v[rows])), f"{what}: v differs in {int(np.sum(eo.bits(v[inside]) != eo.bits(all_v[rows])))} entries"
    assert np.array_equal(eo.bits(c[inside]), eo.bits(all_c[rows])), f"{what}: c differs"


def _sync_scores(o, req):
    """v and c of every row as the synchronous library writes them (the identity the scores form is held to)."""
    kw = {k: val for k, val in req.items() if k not in ("exclude", "topn")}
    return o.sync.scores(**kw)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("d", DIMS)
def test_lists_around_one_tile(d, storage):
    """1, 17 and 4097 rows x every list length around a tile x the list contents and the requests in rotation, so that every
    content meets every length class and every request; rank against the ONLY set and the oracle, scores against the
    synchronous library and the oracle."""
    rng = np.random.default_rng(d)
    k = 0
    for n in (1, 17, 4097):
        feats, table = hc.float_catalogue(n, d)
        with _Opened(feats, table, storage) as o:
            info = o.ct.info()
            t = info["tile_rows"]
            assert t == 2048 // (d // (4 if storage == "f32" else 8)) and (info["rows"], info["dim"], info["borrowed"]) == (n, d, 1)
            assert (info["max_candidates"], info["rank_launches"], info["scores_call_launches"]) == (1 << 20, 4, 1)
            reqs = _requests(n, d)
            vals = [_values(o, r) for r in reqs]
            sync = [_sync_scores(o, r) for r in reqs]
            for (v, c), (sv, sc) in zip(vals, sync):   # the synchronous library is the oracle's: one identity, two references
                assert ec.same_floats(sv, v) and ec.same_floats(sc, c)
            for m in (0, 1, 2, t - 1, t, t + 1, 2 * t + 1):
                lists = _lists(n, m, rng)
                for name in list(lists)[k % 2::2]:
                    i = k % len(reqs)
                    k += 1
                    what = f"{storage} n={n} d={d} m={m} {name} request {i}"
                    before = o.ct.info()["launches"]
                    got = _check_rank(o, vals[i][0], lists[name], reqs[i], what)
                    launched = o.ct.info()["launches"] - before
                    extra = (1 if reqs[i].get("exclude") else 0) + (1 if reqs[i].get("audio_weight", 0.0) != 0.0 else 0)
                    assert launched == (4 + extra if m else 1), f"{what}: {launched} launches"
                    if name == "outside" or m == 0:
                        assert got[2] == 0 and np.all(got[0] == -1)
                    before = o.ct.info()["launches"]
                    _check_scores(o, sync[i][0], sync[i][1], lists[name], reqs[i], what)
                    assert o.ct.info()["launches"] - before == ((1 + (reqs[i].get("audio_weight", 0.0) != 0.0)) if m else 0), f"{what}: scores launches"


@pytest.mark.parametrize("d,storage", [(16, "f32"), (64, "f32"), (16, "fp16"), (64, "bf16")])
def test_every_workgroup_and_one_entry_more(d, storage):
    """65 537 rows: the widest grid the table allows, a list of grid x t + 1 entries (every workgroup one tile, the first a
    second tile of one entry), random with repeats and with hostile ids; topn above the distinct rows of a short list."""
    n = 65537
    rng = np.random.default_rng(7 * d)
    feats, table = hc.float_catalogue(n, d)
    with _Opened(feats, table, storage) as o:
        info = o.ct.info()
        grid, t = info["grid"], info["tile_rows"]
        assert grid > 16
        reqs = _requests(n, d)
        m = grid * t + 1
        lists = _lists(n, m, rng)
        for i, name in ((0, "random"), (1, "hostile"), (2, "reversed"), (3, "random")):
            v, c = _values(o, reqs[i])
            _check_rank(o, v, lists[name], reqs[i], f"{storage} n={n} d={d} m={m} {name} request {i}")
            sv, sc = _sync_scores(o, reqs[i])
            _check_scores(o, sv, sc, lists[name], reqs[i], f"{storage} n={n} d={d} m={m} {name} request {i}")
        few = lists["random"][:300]
        req = dict(reqs[0], topn=1024)
        got = _check_rank(o, _values(o, req)[0], few, req, "topn above the distinct listed rows")
        assert 0 < got[2] <= np.unique(few).size < 1024


def test_a_million_entries():
    """2^20 entries at d = 16 over 65 537 rows: about 16 copies of every row, each ranked once; hostile ids among them."""
    n, d, m = 65537, 16, 1 << 20
    rng = np.random.default_rng(20)
    feats, table = hc.float_catalogue(n, d)
    with _Opened(feats, table, "f32") as o:
        ids = _lists(n, m, rng)["hostile"]
        assert _listed(o, ids).size > n * 0.99
        for req in _requests(n, d)[:2]:
            v, _ = _values(o, req)
            got = _check_rank(o, v, ids, req, f"2^20 entries top-{req['topn']}")
            assert np.unique(got[0][: got[2]]).size == got[2], "a row listed more than once is ranked once"
        sv, sc = _sync_scores(o, req)
        _check_scores(o, sv, sc, ids, req, "2^20 entries")
        user, dev_ids = _dev(np.asarray(req["user"], F32)), _dev(np.concatenate([ids, ids[:1]]))
        with pytest.raises(Exception, match=r"n_candidates 1048577 out of \[0, 1048576\]"):
            o.ct.rank(user, dev_ids)


def test_a_shard_with_a_row_base():
    """Ids, exclusions and answers are global; local rows are not ids."""
    n, d, base = 1500, 32, 1_000_000
    feats, table = ec.catalogue(n, d)
    rng = np.random.default_rng(3)
    with _Opened(feats, table, "f32", row_base=base) as o:
        req = dict(user=bc.users(n, d, 1)[0], metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=3, topn=40,
                   exclude=[base + 7, 7, base + n, base + n - 1, base, -1, base + 7])
        v, _ = _values(o, req)
        sv, sc = _sync_scores(o, req)
        for name, ids in _lists(n, 700, rng, base).items():
            got = _check_rank(o, v, ids, req, f"row_base {name}")
            assert got[2] == 0 or got[0][: got[2]].min() >= base
            _check_scores(o, sv, sc, ids, req, f"row_base {name}")
        local = np.arange(0, 700, dtype=np.int64)   # (local rows are not global ids)
        assert _rank(o, local, req)[2] == 0


def test_rows_that_form_no_key_are_still_scored():
    """The all-zero row (c = 0 under cosine) and, under dot, the rows holding NaN and infinity: no key in rank, their values
    in scores."""
    n, d = 17, 32
    feats, table = ec.catalogue(n, d)
    with _Opened(feats, table, "f32") as o:
        ids = np.array([5, 7, 8, 7, 5, 6, 2], np.int64)
        for metric in ("cosine", "dot"):
            req = dict(user=bc.users(n, d, 1)[0], metric=metric, embed_weight=1.0, topn=10)
            v, c = _values(o, req)
            if metric == "cosine":
                assert c[5] == 0 and v[5] == 0
            else:
                assert np.isnan(v[7]) and np.isinf(v[8])
            got = _check_rank(o, v, ids, req, f"hostile rows, {metric}")
            assert set(got[0][: got[2]].tolist()) == {r for r in (2, 5, 6, 7, 8) if np.isfinite(v[r])}
            sv, sc = _sync_scores(o, req)
            assert ec.same_floats(sv, v)
            _check_scores(o, sv, sc, ids, req, f"hostile rows, {metric}")


# ---- streams ----

def _stream_setup(n=4097, d=32, storage="f32"):
    feats, table = hc.float_catalogue(n, d)
    return _Opened(feats, table, storage)


def test_a_list_made_on_a_side_stream_is_read_in_stream_order():
    import torch
    with _stream_setup() as o:
        req = dict(user=bc.users(o.n, 32, 1, seed=1)[0], metric="cosine", embed_weight=1.0, audio_weight=0.5, audio_row=11, topn=50)
        user = _dev(req["user"])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            big = torch.randn(1 << 22, device="cuda:0")   # (work in front of the list on the side stream)
            ids = torch.topk(big[: o.n] + big[o.n: 2 * o.n], 900).indices.to(torch.int64)   # a first stage's proposal
            kw = {k: val for k, val in req.items() if k != "user"}
            idx, sc, cnt = o.ct.rank(user, ids, stream=side, **kw)
            v, c, flag = o.ct.scores(user, ids, stream=side, **{k: val for k, val in kw.items() if k != "topn"})
        side.synchronize()
        ids = ids.cpu().numpy()
        all_v, _ = _values(o, req)
        _same((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())), _oracle_rank(o, all_v, ids, req), 50, "side stream")
        assert np.array_equal(eo.bits(v.cpu().numpy()), eo.bits(all_v[ids])) and bool(flag.all())


def test_two_streams_alternate_over_one_table():
    """20 enqueues, streams alternating, distinct outputs and lists, no ordering by the caller: the table's event orders the
    claimed list, the bitmap and the audio buffer."""
    import torch
    with _stream_setup() as o:
        users = bc.users(o.n, 32, 20, seed=3)
        rng = np.random.default_rng(1)
        lists = [rng.integers(-2, o.n + 2, 500 + 97 * i) for i in range(20)]
        dev_users, dev_lists = _dev(users), [_dev(x) for x in lists]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        for i in range(20):
            kw = dict(topn=100, metric="dot" if i % 3 else "cosine", embed_weight=1.0)
            if i % 4 == 0:
                kw.update(audio_weight=1.0, audio_row=i)
            outs.append((kw, o.ct.rank(dev_users[i], dev_lists[i], stream=streams[i % 2], **kw)))
        for s in streams:
            s.synchronize()
        for i, (kw, (idx, sc, cnt)) in enumerate(outs):
            req = dict(kw, user=users[i])
            _same((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())), _oracle_rank(o, _values(o, req)[0], lists[i], req), 100, f"enqueue {i}")


def test_preallocated_outputs_allocate_nothing():
    import torch
    with _stream_setup() as o:
        users = bc.users(o.n, 32, 9, seed=4)
        dev_users = _dev(users)
        ids = np.random.default_rng(2).integers(0, o.n, 3000)
        dev_ids, excl = _dev(ids), _dev(np.arange(0, 600, 2, dtype=np.int64))
        ranked = (torch.empty(64, dtype=torch.int64, device="cuda:0"), torch.empty(64, dtype=torch.float32, device="cuda:0"),
                  torch.empty((), dtype=torch.int32, device="cuda:0"))
        valued = (torch.empty(3000, dtype=torch.float32, device="cuda:0"), torch.empty(3000, dtype=torch.float32, device="cuda:0"),
                  torch.empty(3000, dtype=torch.uint8, device="cuda:0"))
        kw = dict(metric="cosine", embed_weight=1.0, audio_weight=1.0, audio_row=5)
        o.ct.rank(dev_users[0], dev_ids, topn=64, exclude=excl, out=ranked, **kw)   # the warm-up calls
        o.ct.scores(dev_users[0], dev_ids, out=valued, **kw)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        for i in range(10):
            got = o.ct.rank(dev_users[i % 9], dev_ids, topn=64, exclude=excl, out=ranked, **kw)
            assert got[0] is ranked[0] and got[1] is ranked[1] and got[2] is ranked[2]
            assert o.ct.scores(dev_users[i % 9], dev_ids, out=valued, **kw)[0] is valued[0]
            assert torch.cuda.memory_allocated() == held, f"call {i} allocated device memory"
        torch.cuda.synchronize()
        req = dict(kw, user=users[0], topn=64, exclude=list(range(0, 600, 2)))
        all_v, _ = _values(o, req)
        _same((ranked[0].cpu().numpy(), ranked[1].cpu().numpy(), int(ranked[2].item())), _oracle_rank(o, all_v, ids, req), 64, "out=")
        assert np.array_equal(eo.bits(valued[0].cpu().numpy()), eo.bits(all_v[ids]))
        with pytest.raises(ValueError, match="out v of shape"):
            o.ct.scores(dev_users[0], dev_ids[:10], out=valued, **kw)


@pytest.mark.parametrize("storage", STORAGES)
def test_a_borrowed_table_rewritten_between_two_enqueues(storage):
    import torch
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_cand import CandidateEmbeddingTable
    n, d = 3000, 32
    feats, table = hc.float_catalogue(n, d)
    t, wide, _ = _table_tensor(table, storage)
    new_t, new_wide, _ = _table_tensor(np.random.default_rng(8).standard_normal((n, d), dtype=F32), storage)
    user = bc.users(n, d, 1)[0]
    ids = np.random.default_rng(9).integers(0, n, 800)
    dev_user, dev_ids = _dev(user), _dev(ids)
    req = dict(topn=30, metric="cosine", embed_weight=1.0, audio_weight=0.25, audio_row=9)
    with CosineEngine(feats) as eng, CandidateEmbeddingTable(eng, t) as ct:
        assert ct.info()["table_dev"] == t.data_ptr() and ct.info()["borrowed"] == 1
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        current = wide.copy()
        for rows in (slice(int(ids[0]), int(ids[0]) + 1), slice(100, 900), slice(0, n)):
            with torch.cuda.stream(s):
                first = ct.rank(dev_user, dev_ids, stream=s, **req)
                t[rows] = new_t[rows]                      # torch rewrites rows on the stream, between two enqueues
                second = ct.rank(dev_user, dev_ids, stream=s, **req)
            s.synchronize()
            for got, rows_now in ((first, current), (second, None)):
                if rows_now is None:
                    current = current.copy()
                    current[rows] = new_wide[rows]
                    rows_now = current
                v, _, _, _ = ec.expected(feats, rows_now, dict(req, user=user))
                only = np.full(n, np.nan, F32)
                only[np.unique(ids)] = v[np.unique(ids)]
                _same((got[0].cpu().numpy(), got[1].cpu().numpy(), int(got[2].item())), eo.topn(only, 30), 30, f"{storage} rows {rows}")


def test_no_claim_survives_a_call():
    """A rank call directly behind a rank call with another list, a hundred times over on one stream without a synchronise
    between them: a claim left standing by one call would make the next drop that row."""
    import torch
    with _stream_setup(n=4097, d=16) as o:
        req = dict(user=bc.users(o.n, 16, 1, seed=5)[0], metric="dot", embed_weight=1.0, topn=1024)
        v, _ = _values(o, req)
        rng = np.random.default_rng(4)
        every = np.arange(o.n, dtype=np.int64)
        lists = [np.concatenate([every, every[::-1]]), every[:1], rng.integers(0, o.n, 5000), every[::-1], np.full(3000, 77, np.int64)] * 20
        user, dev_lists = _dev(req["user"]), [_dev(x) for x in lists[:5]]
        outs = [o.ct.rank(user, dev_lists[i % 5], metric="dot", embed_weight=1.0, topn=1024) for i in range(len(lists))]
        torch.cuda.current_stream().synchronize()
        for i, (idx, sc, cnt) in enumerate(outs):
            _same((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())), _oracle_rank(o, v, lists[i], req), 1024, f"call {i}")


def test_refusals_launch_nothing_and_leave_the_table_answering():
    import torch
    from spotify_recommender_amd import capi
    with _stream_setup() as o:
        user, ids = _dev(bc.users(o.n, 32, 1)[0]), _dev(np.arange(100, dtype=np.int64))
        torch.cuda.synchronize()
        before = o.ct.info()
        bad = [(dict(topn=0), "topn 0 out of"), (dict(topn=1025), "topn 1025 out of"), (dict(embed_weight=0.0), "embed_weight"),
               (dict(audio_weight=9.0), "audio_weight"), (dict(audio_weight=1.0, audio_row=o.n), "needs audio by value or a valid audio_row"),
               (dict(exclude=_dev(np.zeros(1025, np.int64))), "n_exclude 1025 out of")]
        for kw, text in bad:
            with pytest.raises(capi.Mi355Error, match=text):
                o.ct.rank(user, ids, **kw)
        with pytest.raises(capi.Mi355Error, match="user_dev is not 16-byte aligned"):
            o.ct.rank(_dev(np.zeros(33, F32))[1:], ids)
        with pytest.raises(ValueError, match="metric"):
            o.ct.rank(user, ids, metric="l2")
        with pytest.raises(ValueError, match="candidates is a contiguous torch.int64"):
            o.ct.rank(user, ids.to(torch.int32))
        with pytest.raises(ValueError, match="user batches over a list are not served"):
            o.ct.rank(_dev(np.zeros((2, 32), F32)), ids)
        with pytest.raises(NotImplementedError):
            o.ct.query(user)
        L = capi.embed_cand_lib()
        q = capi.EmbedCandQuery(size=78, user_dev=user.data_ptr(), candidates_dev=ids.data_ptr(), n_candidates=100, topn=10, w_embed=1.0)
        out = torch.empty(10, dtype=torch.int64, device="cuda:0")
        res = capi.EmbedStreamResult(size=32, out_idx_dev=out.data_ptr())
        assert L.mi355rec_embed_cand_enqueue_rank(o.ct._e, ctypes.byref(q), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
        assert b"embed cand query of size 78: not the end of a field of the 80 bytes" in L.mi355rec_embed_cand_last_error(o.ct._e)
        q.size = 80
        assert L.mi355rec_embed_cand_enqueue_rank(o.ct._e, ctypes.byref(q), ctypes.byref(capi.EmbedStreamResult(size=32)), None) == capi.ERR_INVALID_ARG
        assert b"null out_idx_dev" in L.mi355rec_embed_cand_last_error(o.ct._e)
        assert L.mi355rec_embed_cand_enqueue_scores(o.ct._e, ctypes.byref(q), ctypes.byref(capi.EmbedCandScores(size=32)), None) == capi.ERR_INVALID_ARG
        assert b"null out_v_dev with n_candidates 100" in L.mi355rec_embed_cand_last_error(o.ct._e)
        q.candidates_dev = None
        assert L.mi355rec_embed_cand_enqueue_rank(o.ct._e, ctypes.byref(q), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
        assert b"null candidate list with n_candidates 100" in L.mi355rec_embed_cand_last_error(o.ct._e)
        q.n_candidates = -1
        assert L.mi355rec_embed_cand_enqueue_rank(o.ct._e, ctypes.byref(q), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
        assert b"n_candidates -1 out of" in L.mi355rec_embed_cand_last_error(o.ct._e)
        after = o.ct.info()
        assert (after["launches"], after["enqueues"], after["scores_launches"]) == (before["launches"], before["enqueues"], before["scores_launches"])
        req = dict(user=bc.users(o.n, 32, 1)[0], metric="cosine", embed_weight=1.0, topn=10)
        _check_rank(o, _values(o, req)[0], np.arange(100, dtype=np.int64), req, "after the refusals")
