"""STREAMED EMBEDDING REQUESTS on the GPU (include/mi355rec_embed_stream.h, csrc/embed_stream.hip.h): what
StreamedEmbeddingTable leaves in device tensors — ids, order, score bits, count, padding — bit for bit against the
synchronous libraries on the same engine (EmbeddingTable, HalfEmbeddingTable, EmbeddingBatchTable) and against
tests/embed_oracle.py, after one stream.synchronize(): both paths at the sizes where the scans can go wrong, exclusion
lists as the prepare kernel must take them (any order, duplicates, foreign and negative ids, -1 padding, 1023 / 1024 ids),
a row base, streams (a user computed by torch on a side stream, two streams over one table, out= without allocation, an
enqueue behind a sleeping kernel), a borrowed table rewritten between enqueues, refusals that launch nothing.  Hostile
means values, never addresses."""
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


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _table_tensor(table, storage):
    """(the device tensor a model would hold, the fp32 table the contract speaks of, what the synchronous library takes)."""
    import torch
    from spotify_recommender_amd.embed_half import to_storage, widen
    if storage == "f32":
        return _dev(table), table, table
    words = to_storage(table, storage)
    t = _dev(words.view(np.int16)).view(torch.float16 if storage == "fp16" else torch.bfloat16)
    return t, widen(words, storage), hc.as_given(words, storage)


def _open(feats, table, storage="f32", **kw):
    """(engine, streamed table over a borrowed tensor, the synchronous table over the same rows, the fp32 rows)."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    eng = CosineEngine(feats, **kw)
    t, wide, given = _table_tensor(table, storage)
    ref = EmbeddingTable(eng, given) if storage == "f32" else HalfEmbeddingTable(eng, given)
    return eng, StreamedEmbeddingTable(eng, t), ref, wide


def _tile_rows(d, storage):
    """The scan's tile, asked of the library (a one-row table)."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    t, _, _ = _table_tensor(np.ones((1, d), F32), storage)
    with CosineEngine(np.ones((1, 12), F32)) as eng, StreamedEmbeddingTable(eng, t) as st:
        tile = st.info()["tile_rows"]
    assert tile == 2048 // (d // (4 if storage == "f32" else 8)) and 64 <= tile <= 1024
    return tile


def _vector_request(req, wide, row_base=0):
    """A request of ec.requests as a vector can express it: members by rows become their in-order sum and join the exclusions."""
    req = dict(req)
    if "rows" in req:
        rows = req.pop("rows")
        req["user"] = eo.user_from_rows(wide, rows)
        req["exclude"] = list(req.get("exclude", [])) + [r + row_base for r in rows]
    return req


def _ask(st, req, stream=None):
    """One streamed request; (idx [topn], score [topn], count) on the host after one synchronise."""
    import torch
    kw = {k: v for k, v in req.items() if k not in ("user", "exclude")}
    excl = _dev(np.asarray(req["exclude"], np.int64)) if req.get("exclude") is not None and len(req["exclude"]) else None
    idx, sc, cnt = st.query(_dev(np.asarray(req["user"], F32)), exclude=excl, stream=stream, **kw)
    (stream or torch.cuda.current_stream()).synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())


def _same_as_sync(got, ref_answer, topn, what):
    idx, sc, cnt = got
    ri, rs = ref_answer
    assert cnt == ri.size, f"{what}: count {cnt}, the synchronous call found {ri.size}"
    assert idx[:cnt].tolist() == ri.tolist(), f"{what}: ids differ (got {idx[:8].tolist()}, want {ri[:8].tolist()})"
    assert np.array_equal(eo.bits(sc[:cnt]), eo.bits(rs)), f"{what}: score bits differ"
    assert idx.shape == (topn,) and np.all(idx[cnt:] == -1) and np.all(eo.bits(sc[cnt:]) == 0), f"{what}: padding"


def _single_requests(n, d, wide):
    reqs = [_vector_request(r, wide) for r in ec.requests(n, d)]
    nan = np.array(reqs[0]["user"], F32)
    nan[d // 2] = np.nan
    reqs.append(dict(user=nan, metric="dot", embed_weight=1.0, topn=10))
    return reqs


def _check_single(st, ref, feats, wide, reqs, what, oracle):
    for i, req in enumerate(reqs):
        got = _ask(st, req)
        _same_as_sync(got, ref.query(**req), req["topn"], f"{what} request {i}")
        if oracle:
            _, _, ids, sc = ec.expected(feats, wide, req)
            assert got[2] == ids.size and got[0][: ids.size].tolist() == ids.tolist() and np.array_equal(eo.bits(got[1][: ids.size]), eo.bits(sc)), \
                f"{what} request {i}: differs from the oracle"
    assert _ask(st, reqs[-1])[2] == 0, "every v of a user with a NaN is NaN under dot: count 0, all padding"


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("d", DIMS)
def test_one_user_equals_the_synchronous_library(d, storage):
    t = _tile_rows(d, storage)
    for n in (1, 17, t - 1, t, t + 1, 4097):
        feats, table = hc.float_catalogue(n, d)
        eng, st, ref, wide = _open(feats, table, storage)
        with eng, st, ref:
            info = st.info()
            assert (info["rows"], info["dim"], info["borrowed"]) == (n, d, 1) and info["grid"] >= 1
            assert info["storage_name"] == {"f32": "fp32"}.get(storage, storage)
            reqs = _single_requests(n, d, wide)
            before = info["launches"]
            _check_single(st, ref, feats, wide, reqs, f"{storage} n={n} d={d}", oracle=n == 4097)
            after = st.info()
            with_audio = sum(1 for r in reqs if r.get("audio_weight", 0.0) != 0.0)
            assert after["enqueues"] == len(reqs) + 1 and after["scores_launches"] == with_audio and after["launches"] > before


@pytest.mark.parametrize("d,storage", [(16, "f32"), (64, "f32"), (16, "fp16"), (64, "bf16")])
def test_many_lists_reach_the_merge(d, storage):
    n = 65537
    feats, table = hc.float_catalogue(n, d)
    eng, st, ref, wide = _open(feats, table, storage)
    with eng, st, ref:
        assert st.info()["grid"] > 16
        _check_single(st, ref, feats, wide, _single_requests(n, d, wide), f"{storage} n={n} d={d}", oracle=False)


def _exclusion_lists(n, rng):
    lists = [[1, 1, 3, n - 1, n, n + 9, 2 ** 31 + 1, 2 ** 40, -1], list(range(min(n, 700) - 1, -1, -1))]
    for L in (0, 1, 2, 3, 1023, 1024):   # dense in duplicates, with foreign and negative ids
        lists.append([int(x) for x in rng.integers(-3, n + 4, L)])
    return lists


@pytest.mark.parametrize("d,storage", [(16, "f32"), (64, "fp16")])
def test_exclusion_lists_in_any_order(d, storage):
    """The prepare kernel's lists against the host's sort + unique: every L that changes the sort's width, a hostile and a
    descending list, every row of a 1024-row table (count 0), every row but one of a 1025-row table."""
    rng = np.random.default_rng(5)
    for n in (1024, 1025, 4097):
        feats, table = hc.float_catalogue(n, d)
        eng, st, ref, wide = _open(feats, table, storage)
        with eng, st, ref:
            lists = _exclusion_lists(n, rng)
            if n <= 1025:
                lists.append([int(x) for x in rng.permutation(n)[:1024]])
            user = rng.standard_normal(d, dtype=F32)
            for i, excl in enumerate(lists):
                for metric, topn in (("cosine", 10), ("dot", 1024)):
                    req = dict(user=user, metric=metric, embed_weight=1.0, topn=topn, exclude=excl)
                    if i == 0:
                        req.update(audio_weight=0.5, audio_row=n // 3)
                    got = _ask(st, req)
                    _same_as_sync(got, ref.query(**req), topn, f"{storage} n={n} d={d} list {i} (L={len(excl)}) {metric}")
                    assert not set(got[0][: got[2]].tolist()) & set(excl)
            if n == 1024:
                assert got[2] == 0 and np.all(got[0] == -1), "every row excluded"
            if n == 1025:
                assert got[2] <= 1, "every row but one excluded"


def _matrix(lists, L):
    """The exclusion matrix of a batch: row b is lists[b] cut to L ids and padded with -1."""
    m = np.full((len(lists), L), -1, np.int64)
    for b, ids in enumerate(lists):
        m[b, : min(len(ids), L)] = ids[:L]
    return m


def _batch_lists(n, B, L, rng):
    """Rows of different true lengths (0 .. L) under the padding: duplicates, foreign ids, -1 in the middle of a row."""
    return [[int(x) for x in rng.integers(-2, n + 3, (7 * b + 3) % (L + 1))] for b in range(B)]


def _ask_batch(st, us, topn, metric, w, lists, L):
    import torch
    excl = _dev(_matrix(lists, L)) if L else None
    idx, sc, cnt = st.query(_dev(us), topn=topn, metric=metric, embed_weight=w, exclude=excl)
    torch.cuda.current_stream().synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()


def _check_batch(st, ref, table, us, topn, metric, w, lists, L, what, row_base=0, oracle_every=1):
    B = len(us)
    before = st.info()["launches"]
    ids, sc, counts = _ask_batch(st, us, topn, metric, w, lists, L)
    assert ids.shape == (B, topn) and sc.shape == (B, topn) and counts.shape == (B,)
    assert st.info()["launches"] - before == 2 + (B % 8 != 0) + 2 * -(-B // 8) + (L > 0), f"{what}: launches"
    seen = [[x for x in row[:L] if x >= 0] for row in lists]   # (the identity: row b with its negative entries dropped)
    ri, rs, rc = ref.query_users(users=us, topn=topn, metric=metric, embed_weight=w, exclude=seen)
    assert np.array_equal(counts, rc) and np.array_equal(ids, ri) and np.array_equal(eo.bits(sc), eo.bits(rs)), \
        f"{what}: differs from EmbeddingBatchTable for users {np.nonzero((ids != ri).any(axis=1) | (counts != rc))[0][:8].tolist()}"
    for b in range(0, B, oracle_every):
        wi, ws, wc = bc.expected(table, us[b], metric, w, topn, seen[b], row_base)
        assert counts[b] == wc and ids[b].tolist() == wi.tolist() and np.array_equal(eo.bits(sc[b]), eo.bits(ws)), f"{what} user {b}: differs from the oracle"
    return ids, sc, counts


def _open_batch(feats, table, **kw):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    eng = CosineEngine(feats, **kw)
    return eng, StreamedEmbeddingTable(eng, _dev(table)), EmbeddingBatchTable(eng, table)


@pytest.mark.parametrize("d", [16, 128])
def test_batches_equal_the_synchronous_library_and_the_oracle(d):
    """Every row count x every B below 1024; (topn, L, metric, weight) cycle, so that every topn meets every L."""
    t = _tile_rows(d, "f32")
    rng = np.random.default_rng(d)
    k = 0
    for n in (1, 17, t - 1, t, t + 1, 4097):
        feats, table = ec.catalogue(n, d)
        eng, st, ref = _open_batch(feats, table)
        with eng, st, ref:
            for B in (1, 7, 8, 9, 16, 17):
                topn = (1, 10, 128, min(n + 5, 128))[k % 4]
                L = (0, 1, 5, 1024)[(k // 4 + k) % 4]
                metric, w = (("cosine", 1.0), ("dot", -0.5), ("cosine", 4.0))[k % 3]
                k += 1
                _check_batch(st, ref, table, bc.users(n, d, B), topn, metric, w, _batch_lists(n, B, L, rng), L, f"n={n} d={d} B={B} top-{topn} L={L}")


@pytest.mark.parametrize("d", DIMS)
def test_batches_at_4097_rows_every_dim(d):
    n = 4097
    rng = np.random.default_rng(100 + d)
    feats, table = ec.catalogue(n, d)
    eng, st, ref = _open_batch(feats, table)
    with eng, st, ref:
        for B, topn, L, metric in ((9, 10, 5, "cosine"), (17, 128, 1024, "dot"), (8, 1, 1, "cosine"), (7, 128, 0, "dot")):
            _check_batch(st, ref, table, bc.users(n, d, B, seed=2), topn, metric, 1.0, _batch_lists(n, B, L, rng), L, f"n={n} d={d} B={B}")


@pytest.mark.parametrize("n,d", [(17, 16), (4097, 16), (1000, 128)])
def test_a_thousand_and_twenty_four_users(n, d):
    B = 1024
    rng = np.random.default_rng(n + d)
    feats, table = ec.catalogue(n, d)
    eng, st, ref = _open_batch(feats, table)
    with eng, st, ref:
        L = 5 if n != 4097 else 1024
        _check_batch(st, ref, table, bc.users(n, d, B), 10 if n != 17 else 128, "cosine", 1.0, _batch_lists(n, B, L, rng), L, f"n={n} d={d} B={B}",
                     oracle_every=101)


@pytest.mark.parametrize("metric", bc.METRICS)
@pytest.mark.parametrize("n,d", [(1000, 16), (4097, 16), (4097, 64)])
def test_one_pass_mixes_users_that_do_not_influence_each_other(n, d, metric):
    """tests/test_gpu_embed_batch.py's mixed pass — ordinary, zero, huge, tiny, NaN and fully excluded users — with lists cut to 1024."""
    from tests.test_gpu_embed_batch import _mixed
    feats, table = ec.catalogue(n, d)
    us, lists = _mixed(n, d)
    lists = [x[:1024] for x in lists]
    eng, st, ref = _open_batch(feats, table)
    with eng, st, ref:
        for topn, w in ((10, 1.0), (128, -0.5)):
            ids, sc, counts = _check_batch(st, ref, table, us, topn, metric, w, lists, 1024, f"mixed n={n} d={d} {metric}")
            assert ids[0].tolist() == ids[1].tolist() and counts[0] == counts[1]
            if metric == "dot":
                assert counts[5] == 0 and np.all(ids[5] == -1) and np.all(sc[5] == 0), "every v of a user with a NaN is NaN"
            if n <= 1024:
                assert counts[6] == 0 and np.all(ids[6] == -1), "a user who excludes every row"


def test_a_shard_with_a_row_base():
    """One shard of a larger catalogue on both paths: ids and exclusions are global."""
    n, d, base = 1500, 32, 1_000_000
    feats, table = ec.catalogue(n, d)
    eng, st, ref, wide = _open(feats, table, "f32", row_base=base)
    with eng, st, ref:
        user = bc.users(n, d, 1)[0]
        for excl in ([base + 7, 7, base + n, base + n - 1, base, -1, base + 7], [base + r for r in range(1024)], []):
            req = dict(user=user, metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=3, topn=40, exclude=excl)
            got = _ask(st, req)
            _same_as_sync(got, ref.query(**req), 40, f"row_base, {len(excl)} ids")
            _, _, ids, sc = ec.expected(feats, wide, req, base)
            assert got[0][: ids.size].tolist() == ids.tolist() and np.array_equal(eo.bits(got[1][: ids.size]), eo.bits(sc))
            assert got[2] and got[0][: got[2]].min() >= base and not set(got[0].tolist()) & set(excl)
    from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
    eng, st, ref, _ = _open(feats, table, "f32", row_base=base)
    with eng, st, ref, EmbeddingBatchTable(eng, table) as bref:
        lists = [[base + 7, 7, base + n, base + (3 * b) % n] for b in range(9)]
        lists[4] = []
        _check_batch(st, bref, table, bc.users(n, d, 9), 40, "cosine", 0.5, lists, 4, "row_base batch", row_base=base)


# ---- streams ----

def _stream_setup(n=4097, d=32, storage="f32"):
    feats, table = hc.float_catalogue(n, d)
    return (feats, table) + _open(feats, table, storage)


def test_a_user_computed_on_a_side_stream_is_read_in_stream_order():
    import torch
    feats, table, eng, st, ref, wide = _stream_setup()
    with eng, st, ref:
        a, b = _dev(bc.users(4097, 32, 2, seed=1))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            big = torch.randn(1 << 22, device="cuda:0")   # (work in front of the user on the side stream)
            user = a * 2.0 + b + 0.0 * big[:32]
            idx, sc, cnt = st.query(user, topn=50, metric="cosine", embed_weight=1.0, audio_weight=0.5, audio_row=11, stream=side)
        side.synchronize()
        want = ref.query(user=user.cpu().numpy(), topn=50, metric="cosine", embed_weight=1.0, audio_weight=0.5, audio_row=11)
        _same_as_sync((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())), want, 50, "side stream")


def test_two_streams_alternate_over_one_table():
    """20 enqueues, streams alternating, distinct outputs, no ordering by the caller: the table's event orders its buffers."""
    import torch
    feats, table, eng, st, ref, wide = _stream_setup()
    with eng, st, ref:
        users = bc.users(4097, 32, 20, seed=3)
        excl = [int(x) for x in np.random.default_rng(1).integers(0, 4097, 300)]
        dev_users, dev_excl = _dev(users), _dev(np.asarray(excl, np.int64))
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        for i in range(20):
            kw = dict(topn=100, metric="dot" if i % 3 else "cosine", embed_weight=1.0, exclude=dev_excl if i % 2 else None)
            if i % 4 == 0:
                kw.update(audio_weight=1.0, audio_row=i)
            outs.append((kw, st.query(dev_users[i], stream=streams[i % 2], **kw)))
        for s in streams:
            s.synchronize()
        for i, (kw, (idx, sc, cnt)) in enumerate(outs):
            kw = dict(kw, exclude=excl if i % 2 else None)
            _same_as_sync((idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())), ref.query(user=users[i], **kw), 100, f"enqueue {i}")
        # ... and a batch on one stream behind a single request on the other
        from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
        with EmbeddingBatchTable(eng, table) as bref:
            one = st.query(dev_users[0], topn=10, stream=streams[0])
            many = st.query(dev_users[:9], topn=10, stream=streams[1])
            again = st.query(dev_users[1], topn=10, stream=streams[0])
            for s in streams:
                s.synchronize()
            ri, rs, rc = bref.query_users(users=users[:9], topn=10)
            assert np.array_equal(many[0].cpu().numpy(), ri) and np.array_equal(eo.bits(many[1].cpu().numpy()), eo.bits(rs))
            for got, u in ((one, users[0]), (again, users[1])):
                _same_as_sync((got[0].cpu().numpy(), got[1].cpu().numpy(), int(got[2].item())), ref.query(user=u, topn=10), 10, "beside a batch")


def test_preallocated_outputs_allocate_nothing():
    import torch
    feats, table, eng, st, ref, wide = _stream_setup()
    with eng, st, ref:
        users = bc.users(4097, 32, 9, seed=4)
        dev_users = _dev(users)
        excl = _dev(np.arange(0, 600, 2, dtype=np.int64))
        one = (torch.empty(64, dtype=torch.int64, device="cuda:0"), torch.empty(64, dtype=torch.float32, device="cuda:0"),
               torch.empty((), dtype=torch.int32, device="cuda:0"))
        many = (torch.empty((9, 64), dtype=torch.int64, device="cuda:0"), torch.empty((9, 64), dtype=torch.float32, device="cuda:0"),
                torch.empty(9, dtype=torch.int32, device="cuda:0"))
        kw = dict(topn=64, metric="cosine", embed_weight=1.0)
        st.query(dev_users[0], exclude=excl, audio_weight=1.0, audio_row=5, out=one, **kw)   # the warm-up call
        st.query(dev_users, out=many, **kw)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        for i in range(10):
            got = st.query(dev_users[i % 9], exclude=excl, audio_weight=1.0, audio_row=5, out=one, **kw)
            assert got[0] is one[0] and got[1] is one[1] and got[2] is one[2]
            st.query(dev_users, out=many, **kw)
            assert torch.cuda.memory_allocated() == held, f"call {i} allocated device memory"
        torch.cuda.synchronize()
        want = ref.query(user=users[0], exclude=list(range(0, 600, 2)), audio_weight=1.0, audio_row=5, **kw)
        _same_as_sync((one[0].cpu().numpy(), one[1].cpu().numpy(), int(one[2].item())), want, 64, "out=")
        for b in range(9):
            wi, ws, wc = bc.expected(table, users[b], "cosine", 1.0, 64)
            assert many[0][b].cpu().tolist() == wi.tolist() and int(many[2][b]) == wc
        with pytest.raises(ValueError, match="out idx of shape"):
            st.query(dev_users[0], out=(many[0], one[1], one[2]), **kw)


def test_an_enqueue_does_not_wait_for_the_stream():
    """A kernel that spins for milliseconds stands on the stream; the enqueue behind it returns while it still runs."""
    import torch
    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is missing")
    feats, table, eng, st, ref, wide = _stream_setup()
    with eng, st, ref:
        users = bc.users(4097, 32, 8, seed=6)
        dev_users = _dev(users)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            # 5e6 ticks of the counter the spin reads: 50 ms at the 100 MHz of a constant-rate counter and still 2 ms at a
            # 2.4 GHz shader clock, against the tens of microseconds an enqueue call takes on the host
            torch.cuda._sleep(5_000_000)
            one = st.query(dev_users[0], topn=20, audio_weight=1.0, audio_row=2, stream=s)
            many = st.query(dev_users, topn=20, stream=s)
        assert not s.query(), "the calls returned after the stream had drained: they waited"
        s.synchronize()
        _same_as_sync((one[0].cpu().numpy(), one[1].cpu().numpy(), int(one[2].item())), ref.query(user=users[0], topn=20, audio_weight=1.0, audio_row=2),
                      20, "behind a sleep")
        for b in range(8):
            wi, ws, wc = bc.expected(table, users[b], "cosine", 1.0, 20)
            assert many[0][b].cpu().tolist() == wi.tolist() and int(many[2][b]) == wc


# ---- a borrowed table ----

@pytest.mark.parametrize("storage", STORAGES)
def test_a_borrowed_table_is_the_callers_memory(storage):
    import torch
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    n, d = 3000, 32
    feats, table = hc.float_catalogue(n, d)
    t, wide, given = _table_tensor(table, storage)
    new_t, new_wide, new_given = _table_tensor(np.random.default_rng(8).standard_normal((n, d), dtype=F32), storage)
    kept = t.clone()
    user = bc.users(n, d, 1)[0]
    dev_user = _dev(user)
    req = dict(topn=30, metric="cosine", embed_weight=1.0, audio_weight=0.25, audio_row=9)
    with CosineEngine(feats) as eng:
        st = StreamedEmbeddingTable(eng, t)
        info = st.info()
        assert info["table_dev"] == t.data_ptr() and info["borrowed"] == 1
        copied = StreamedEmbeddingTable(eng, wide if storage == "f32" else given) if storage != "bf16" else None
        if copied is not None:   # the same work buffers and, copied, the table on top of them
            assert copied.info()["borrowed"] == 0 and copied.info()["table_dev"] != t.data_ptr()
            assert copied.info()["device_bytes"] - info["device_bytes"] == t.numel() * t.element_size()
            copied.close()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        current = wide.copy()
        for rows in (slice(1, 2), slice(100, 200), slice(0, n)):
            with torch.cuda.stream(s):
                first = st.query(dev_user, stream=s, **req)
                t[rows] = new_t[rows]                      # torch rewrites rows on the stream, between two enqueues
                second = st.query(dev_user, stream=s, **req)
            s.synchronize()
            for got, rows_now in ((first, current), (second, None)):
                if rows_now is None:
                    current = current.copy()
                    current[rows] = new_wide[rows]
                    rows_now = current
                _, _, ids, sc = ec.expected(feats, rows_now, dict(req, user=user))
                _same_as_sync((got[0].cpu().numpy(), got[1].cpu().numpy(), int(got[2].item())), (ids, sc), 30, f"{storage} rows {rows}")
        # ... what a fresh table over the new values answers
        with StreamedEmbeddingTable(eng, new_t) as fresh:
            a, b = st.query(dev_user, **req), fresh.query(dev_user, **req)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
        after = t.clone()
        st.close()
        del st
        torch.cuda.synchronize()
        assert torch.equal(t.view(torch.int16 if storage != "f32" else torch.int32), after.view(torch.int16 if storage != "f32" else torch.int32)), \
            "closing the table left the tensor as it was"
        assert not torch.equal(t.view(torch.int16 if storage != "f32" else torch.int32), kept.view(torch.int16 if storage != "f32" else torch.int32))


def test_tables_that_are_refused():
    import torch
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    n, d = 40, 16
    feats, table = ec.catalogue(n, d)
    with CosineEngine(feats) as eng:
        wide = _dev(np.zeros((n, 2 * d), F32))
        with pytest.raises(ValueError, match="a borrowed table is contiguous"):
            StreamedEmbeddingTable(eng, wide[:, :d])
        with pytest.raises(ValueError, match="a borrowed table is contiguous"):
            StreamedEmbeddingTable(eng, _dev(np.zeros((d, n), F32)).t())
        with pytest.raises(ValueError, match=r"torch.float64 tensor on cpu: a torch table is a CUDA tensor"):
            StreamedEmbeddingTable(eng, torch.zeros((n, d), dtype=torch.float64))
        with pytest.raises(ValueError, match="dtype torch.float64"):
            StreamedEmbeddingTable(eng, torch.zeros((n, d), dtype=torch.float64, device="cuda:0"))
        with pytest.raises(ValueError, match="a borrowed table of 24 columns"):
            StreamedEmbeddingTable(eng, _dev(np.zeros((n, 24), F32)))
        with pytest.raises(capi.Mi355Error, match="table of 39 rows for a handle of 40 rows"):
            StreamedEmbeddingTable(eng, _dev(table[:39]))
        # the raw call: host memory is not a borrowed table, an odd address is not one either
        L = capi.embed_stream_lib()
        e = ctypes.c_void_p()
        assert L.mi355rec_embed_stream_create_device(eng._h, table.ctypes.data_as(ctypes.c_void_p), n, d, capi.EMBED_STREAM_FP32,
                                                     ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"table_dev is not" in L.mi355rec_embed_stream_last_error(None)
        t = _dev(np.zeros(n * d + 4, F32))
        assert L.mi355rec_embed_stream_create_device(eng._h, ctypes.c_void_p(t.data_ptr() + 8), n, d, capi.EMBED_STREAM_FP32,
                                                     ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"16-byte aligned" in L.mi355rec_embed_stream_last_error(None)
        # a numpy table is copied (and padded, as the other libraries do): the answers are the fp32 library's
        from spotify_recommender_amd.embed import EmbeddingTable
        with StreamedEmbeddingTable(eng, table[:, :10]) as st, EmbeddingTable(eng, table[:, :10]) as ref:
            assert (st.user_dim, st.dim, st.info()["borrowed"]) == (10, 16, 0)
            user = np.zeros(16, F32)
            user[:10] = 1.0
            _same_as_sync(_ask(st, dict(user=user, topn=5)), ref.query(user=user, topn=5), 5, "a copied table")


def test_a_table_on_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_stream import StreamedEmbeddingTable
    feats, table = ec.catalogue(40, 16)
    with CosineEngine(feats) as eng:
        with pytest.raises(ValueError, match="a table on cuda:1 for an engine on cuda:0"):
            StreamedEmbeddingTable(eng, torch.from_numpy(table).to("cuda:1"))


def test_refusals_launch_nothing_and_leave_the_table_answering():
    import torch
    from spotify_recommender_amd import capi
    n, d = 40, 16
    feats, table = ec.catalogue(n, d)
    eng, st, ref, wide = _open(feats, table)
    with eng, st, ref:
        user = bc.users(n, d, 1)[0]
        u, us = _dev(user), _dev(bc.users(n, d, 3))
        _same_as_sync(_ask(st, dict(user=user, topn=5)), ref.query(user=user, topn=5), 5, "before the refusals")
        before = st.info()
        ids = _dev(np.zeros(1025, np.int64))
        refusals = [
            (dict(user=u, topn=0), r"topn 0 out of \[1, 1024\]"),
            (dict(user=u, topn=1025), r"topn 1025 out of \[1, 1024\]"),
            (dict(user=u, embed_weight=0.0), "embed_weight 0: finite, not 0 and at most 4"),
            (dict(user=u, embed_weight=float("nan")), "embed_weight nan"),
            (dict(user=u, audio_weight=4.5, audio_row=1), "audio_weight 4.5"),
            (dict(user=u, audio_weight=1.0), "needs audio by value or a valid audio_row, got row -1"),
            (dict(user=u, audio_weight=1.0, audio_row=n), "got row 40"),
            (dict(user=u, exclude=ids), r"n_exclude 1025 out of \[0, 1024\]"),
            (dict(user=us, topn=0), r"topn 0 out of \[1, 128\]"),
            (dict(user=us, topn=129), r"topn 129 out of \[1, 128\]"),
            (dict(user=_dev(np.zeros((1025, d), F32))), r"n_users 1025 out of \[1, 1024\]"),
            (dict(user=us, exclude=_dev(np.zeros((3, 1025), np.int64))), r"exclude_len 1025 out of \[0, 1024\]"),
            (dict(user=us, embed_weight=-4.5), "embed_weight -4.5"),
        ]
        for kw, text in refusals:
            with pytest.raises(capi.Mi355Error, match=text) as err:
                st.query(kw.pop("user"), **kw)
            assert err.value.code == capi.ERR_INVALID_ARG, text
        for kw, text in ((dict(user=_dev(np.zeros(d + 1, F32))), "user of 17 columns"), (dict(user=user), "user is a CUDA tensor"),
                         (dict(user=u, metric="l2"), "metric 'l2'"), (dict(user=us, audio_weight=1.0, audio_row=0), "a batch of users has no audio side"),
                         (dict(user=u, exclude=_dev(np.zeros((1, 4), np.int64))), "exclude of shape")):
            with pytest.raises(ValueError, match=text):
                st.query(kw.pop("user"), **kw)
        # the raw calls: sizes that do not end a field, flags, a metric, a NULL out_idx_dev, an unaligned user
        L = capi.embed_stream_lib()
        out = torch.empty(5, dtype=torch.int64, device="cuda:0")
        res = capi.EmbedStreamResult(size=32, out_idx_dev=out.data_ptr())
        q = capi.EmbedStreamQuery(size=64, user_dev=u.data_ptr(), audio_row=-1, topn=5, w_embed=1.0)
        for size in (0, 62, 68):
            q.size = size
            assert L.mi355rec_embed_stream_enqueue_query(st._e, ctypes.byref(q), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
            assert b"embed stream query of size %d: not the end of a field of the 64 bytes" % size in L.mi355rec_embed_stream_last_error(st._e)
        for field, value, text in (("flags", 1, b"flags 0x1"), ("metric", 2, b"metric 2"), ("reserved", 3, b"reserved 0x3"),
                                   ("user_dev", u.data_ptr() + 4, b"user_dev is not 16-byte aligned"), ("user_dev", None, b"null user_dev")):
            q = capi.EmbedStreamQuery(size=64, user_dev=u.data_ptr(), audio_row=-1, topn=5, w_embed=1.0)
            setattr(q, field, value)
            assert L.mi355rec_embed_stream_enqueue_query(st._e, ctypes.byref(q), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
            assert text in L.mi355rec_embed_stream_last_error(st._e)
        q = capi.EmbedStreamQuery(size=64, user_dev=u.data_ptr(), audio_row=-1, topn=5, w_embed=1.0)
        assert L.mi355rec_embed_stream_enqueue_query(st._e, ctypes.byref(q), ctypes.byref(capi.EmbedStreamResult(size=32)), None) == capi.ERR_INVALID_ARG
        assert b"null out_idx_dev" in L.mi355rec_embed_stream_last_error(st._e)
        uq = capi.EmbedStreamUsers(size=48, users_dev=us.data_ptr(), n_users=0, topn=5, w_embed=1.0)
        assert L.mi355rec_embed_stream_enqueue_users(st._e, ctypes.byref(uq), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
        assert b"n_users 0 out of [1, 1024]" in L.mi355rec_embed_stream_last_error(st._e)
        uq = capi.EmbedStreamUsers(size=46, users_dev=us.data_ptr(), n_users=3, topn=5, w_embed=1.0)
        assert L.mi355rec_embed_stream_enqueue_users(st._e, ctypes.byref(uq), ctypes.byref(res), None) == capi.ERR_INVALID_ARG
        assert b"embed stream users of size 46" in L.mi355rec_embed_stream_last_error(st._e)
        info = capi.EmbedStreamInfo(size=72)
        assert L.mi355rec_embed_stream_info(st._e, ctypes.byref(info)) == capi.ERR_INVALID_ARG
        after = st.info()
        assert (after["launches"], after["enqueues"], after["scores_launches"]) == (before["launches"], before["enqueues"], before["scores_launches"]), \
            "a refused call launches nothing"
        # out_score_dev and out_count_dev are optional, and the table still answers
        q = capi.EmbedStreamQuery(size=60, user_dev=u.data_ptr(), audio_row=-1, topn=5, w_embed=1.0)   # (a struct that ends at w_embed)
        assert L.mi355rec_embed_stream_enqueue_query(st._e, ctypes.byref(q), ctypes.byref(res), None) == capi.OK
        torch.cuda.synchronize()
        assert out.cpu().tolist() == ref.query(user=user, topn=5)[0].tolist()
        _same_as_sync(_ask(st, dict(user=user, topn=40, metric="dot", embed_weight=2.0)), ref.query(user=user, topn=40, metric="dot", embed_weight=2.0), 40,
                      "after the refusals")
    # a half table serves no batch
    eng, st, ref, _ = _open(feats, table, "fp16")
    with eng, st, ref:
        with pytest.raises(capi.Mi355Error, match="user batches are served over fp32 tables"):
            st.query(_dev(bc.users(n, d, 3)), topn=5)
        assert st.info()["launches"] == 0
