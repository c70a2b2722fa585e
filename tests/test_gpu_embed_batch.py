"""USER BATCHES on the GPU (include/mi355rec_embed_batch.h, csrc/embed_batch.hip.h): embed_batch_scan_kernel's answers,
per user and bit for bit, against tests/embed_oracle.py at the sizes where the kernel can go wrong — the
rows-per-wave-instruction edges of every dim, one tile more or less, several workgroups, many per-workgroup lists in the
merge — crossed with batches that fill a pass, leave a short last pass and cross the pass boundary; one pass that mixes
ordinary, hostile and fully excluded users; the single-user library's answers on the same engine; member rows; a shard with
a row base.  Hostile means values, never addresses."""
import ctypes

import numpy as np
import pytest

from tests import embed_batch_cases as bc
from tests import embed_cases as ec
from tests import embed_oracle as eo

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = [16, 32, 64, 128]


def _open(feats, table, **kw):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_batch import EmbeddingBatchTable
    eng = CosineEngine(feats, **kw)
    return eng, EmbeddingBatchTable(eng, table)


def _tile_rows(d):
    """The scan's tile, asked of the library (a one-row table)."""
    eng, tab = _open(np.ones((1, 12), F32), np.ones((1, d), F32))
    with eng, tab:
        return tab.info()["tile_rows"]


def _sizes(group, d):
    if group == "edges":
        return [1, 2, 3, 4, 5, 15, 16, 17]
    if group == "tile":
        t = _tile_rows(d)
        assert t == 2048 // (d // 4)
        return [t - 1, t, t + 1]
    return [4097] if group == "blocks" else [65537]


@pytest.mark.parametrize("group", ["edges", "tile", "blocks", "many"])
@pytest.mark.parametrize("d", DIMS)
def test_batches_match_the_oracle(d, group):
    """Every n of the group x every B; (metric, weight, topn) cycle through all 24 combinations, and at 4097 rows every
    combination is asked of a batch that crosses the pass boundary."""
    k = 0
    for n in _sizes(group, d):
        feats, table = ec.catalogue(n, d)
        eng, tab = _open(feats, table)
        with eng, tab:
            info = tab.info()
            assert (info["rows"], info["dim"]) == (n, d) and info["device"] >= 0 and info["grid"] >= 1
            assert info["pass_users"] in (1, 2, 4, 8) and info["passes"] == 0 and info["users_served"] == 0
            cs = bc.combos(n)
            for B in bc.BATCHES:
                metric, w, topn = cs[(7 * k) % len(cs)]
                k += 1
                bc.check(tab, table, bc.users(n, d, B), topn=topn, metric=metric, embed_weight=w, exclude=bc.sweep_lists(n, B), what=f"n={n} d={d}")
            if group == "blocks":
                us = bc.users(n, d, 9, seed=1)
                for metric, w, topn in cs:
                    bc.check(tab, table, us, topn=topn, metric=metric, embed_weight=w, what=f"n={n} d={d} every combination")


def _mixed(n, d):
    """Eight users for one pass and their exclusion lists."""
    reqs = ec.requests(n, d)
    normal, huge, tiny = reqs[0]["user"], reqs[5]["user"], reqs[6]["user"]
    nan = normal.copy()
    nan[d // 2] = np.nan
    other = bc.users(n, d, 1, seed=5)[0]
    hostile_list = [1, 1, 3, n - 1, n, n + 9, 2 ** 31 + 1, 2 ** 40, -1]
    long_list = list(range(0, 2 * 5000, 2)) if n > 10_000 else [2, 4, 6]
    us = np.stack([normal, normal, np.zeros(d, F32), huge, tiny, nan, normal, other])
    everything = list(range(min(n, 65536)))   # (the longest list a user may bring: at 65537 rows the last row is left)
    lists = [hostile_list, hostile_list, [], [0, 5, 6], [], [7], everything, long_list]
    return us, lists


@pytest.mark.parametrize("metric", bc.METRICS)
@pytest.mark.parametrize("n,d", [(4097, 16), (4097, 32), (4097, 64), (4097, 128), (65537, 16), (65537, 64)])
def test_one_pass_mixes_users_that_do_not_influence_each_other(n, d, metric):
    feats, table = ec.catalogue(n, d)
    us, lists = _mixed(n, d)
    eng, tab = _open(feats, table)
    with eng, tab:
        for topn, w in ((10, 1.0), (128, -0.5)):
            ids, sc, counts = bc.check(tab, table, us, topn=topn, metric=metric, embed_weight=w, exclude=lists, what=f"mixed n={n} d={d}")
            assert ids[0].tolist() == ids[1].tolist() and np.array_equal(eo.bits(sc[0]), eo.bits(sc[1])) and counts[0] == counts[1]
            if metric == "dot":   # (under cosine a NaN norm fails `den > 1e-8`: c = 0, as for the single call)
                assert counts[5] == 0 and np.all(ids[5] == -1) and np.all(sc[5] == 0), "every v of a user with a NaN is NaN"
            if n <= 65536:
                assert counts[6] == 0 and np.all(ids[6] == -1), "a user who excludes every row"
            else:
                assert counts[6] == 1 and ids[6, 0] == n - 1, "a user who excludes every row but the last"
            if n > 10_000:
                assert not set(ids[7][: counts[7]].tolist()) & set(lists[7])
            for b in range(len(us)):   # ... and what each user gets alone
                ai, asc, ac = tab.query_users(users=us[b : b + 1], topn=topn, metric=metric, embed_weight=w, exclude=[lists[b]])
                assert ai[0].tolist() == ids[b].tolist() and np.array_equal(eo.bits(asc[0]), eo.bits(sc[b])) and ac[0] == counts[b], (b, topn)


@pytest.mark.parametrize("d", DIMS)
def test_the_batch_equals_the_single_call_per_user(d):
    from spotify_recommender_amd.embed import EmbeddingTable
    n = 20_011
    feats, table = ec.catalogue(n, d)
    us = bc.users(n, d, 11)
    lists = bc.sweep_lists(n, 11)
    eng, tab = _open(feats, table)
    with eng, tab, EmbeddingTable(eng, table) as single:
        for metric, w, topn in (("cosine", 1.0, 128), ("dot", -0.5, 10)):
            ids, sc, counts = tab.query_users(users=us, topn=topn, metric=metric, embed_weight=w, exclude=lists)
            for b in range(len(us)):
                si, ss = single.query(user=us[b], metric=metric, embed_weight=w, audio_weight=0.0, topn=topn, exclude=lists[b])
                assert counts[b] == si.size and ids[b, : si.size].tolist() == si.tolist() and np.all(ids[b, si.size:] == -1), (d, metric, b)
                assert np.array_equal(eo.bits(sc[b, : si.size]), eo.bits(ss)) and np.all(sc[b, si.size:] == 0)


def test_member_rows_form_the_users_and_are_excluded_by_default():
    n, d = 5003, 64
    feats, table = ec.catalogue(n, d)
    rng = np.random.default_rng(3)
    rows = [[17], [40, 2, 4000], [int(x) for x in rng.integers(0, n, 32)], [40, 2, 4000]]
    us = np.stack([eo.user_from_rows(table, r) for r in rows])
    eng, tab = _open(feats, table)
    with eng, tab:
        for metric in bc.METRICS:
            ids, sc, counts = tab.query_users(rows=rows, topn=50, metric=metric, embed_weight=1.0, exclude=[[], [99, 100], [], []])
            kept, _, _ = tab.query_users(rows=rows, topn=50, metric=metric, embed_weight=1.0, exclude_rows=False)
            for b, members in enumerate(rows):
                extra = [99, 100] if b == 1 else []
                wi, ws, wc = bc.expected(table, us[b], metric, 1.0, 50, members + extra)
                assert ids[b].tolist() == wi.tolist() and np.array_equal(eo.bits(sc[b]), eo.bits(ws)) and counts[b] == wc, (metric, b)
                assert not set(ids[b].tolist()) & set(members)
                assert kept[b].tolist() == bc.expected(table, us[b], metric, 1.0, 50)[0].tolist()
            assert set(kept[0].tolist()) & {17}, "cosine or dot, a row is among its own best unless it is excluded"


def test_a_narrow_table_is_zero_padded():
    n = 3000
    feats, wide = ec.catalogue(n, 32)
    wide[:, 20:] = 0
    us = bc.users(n, 32, 5)
    us[:, 20:] = 0
    eng, tab = _open(feats, wide[:, :20])
    with eng, tab:
        assert (tab.user_dim, tab.dim) == (20, 32) and tab.info()["dim"] == 32
        ids, sc, counts = tab.query_users(users=us[:, :20], topn=25, metric="cosine", embed_weight=1.0)
        for b in range(5):
            wi, ws, wc = bc.expected(wide, us[b], "cosine", 1.0, 25)
            assert ids[b].tolist() == wi.tolist() and np.array_equal(eo.bits(sc[b]), eo.bits(ws)) and counts[b] == wc


def test_a_shard_with_a_row_base():
    """A single handle that is one shard of a larger catalogue: ids and exclusions are global, member rows local."""
    n, d, base = 1500, 32, 1_000_000
    feats, table = ec.catalogue(n, d)
    us = bc.users(n, d, 9)
    lists = [[base + 7, 7, base + n, base + (3 * b) % n] for b in range(9)]
    lists[4] = []
    eng, tab = _open(feats, table, row_base=base)
    with eng, tab:
        bc.check(tab, table, us, topn=40, metric="cosine", embed_weight=0.5, exclude=lists, row_base=base, what="row_base")
        rows = [[3, 4, 5], [9]]
        ids, sc, counts = tab.query_users(rows=rows, topn=40, metric="dot", embed_weight=1.0)
        for b, members in enumerate(rows):
            wi, ws, wc = bc.expected(table, eo.user_from_rows(table, members), "dot", 1.0, 40, [base + r for r in members], base)
            assert ids[b].tolist() == wi.tolist() and np.array_equal(eo.bits(sc[b]), eo.bits(ws)) and counts[b] == wc


def test_a_million_rows_many_lists():
    """1 000 003 rows at d = 16, eight users: every workgroup of the grid hands a list per user to the merge, top-10 and top-128."""
    n, d = 1_000_003, 16
    rng = np.random.default_rng(9)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    table[123_456] = table[7]
    us = rng.standard_normal((8, d), dtype=F32)
    us[3] = table[7]
    lists = [[], [7, 7, n + 1], [], [123_456], [], [], list(range(0, 60_000, 3)), []]
    eng, tab = _open(feats, table)
    with eng, tab:
        assert tab.info()["grid"] > 64
        bc.check(tab, table, us, topn=10, metric="cosine", embed_weight=1.0, exclude=lists, what="top-10")
        bc.check(tab, table, us, topn=128, metric="dot", embed_weight=-0.5, exclude=lists, what="top-128")


def test_refusals_leave_the_table_answering():
    from spotify_recommender_amd import capi
    n, d = 40, 16
    feats, table = ec.catalogue(n, d)
    us = bc.users(n, d, 3)
    eng, tab = _open(feats, table)
    with eng, tab:
        L = capi.embed_batch_lib()
        # create: a dim the library does not serve (the Python layer would pad it: the raw call), rows that do not match the handle
        for dim, rows, text in ((24, n, b"embedding dim 24: 16, 32, 64 or 128"), (16, n - 1, b"table of 39 rows for a handle of 40 rows")):
            e = ctypes.c_void_p()
            raw = np.zeros((n, dim), F32)
            assert L.mi355rec_embed_batch_create(eng._h, raw.ctypes.data_as(ctypes.c_void_p), rows, dim, ctypes.byref(e)) == capi.ERR_INVALID_ARG
            assert not e and text in L.mi355rec_embed_batch_last_error(None)
        refusals = [
            (dict(users=np.zeros((1025, d), F32)), r"n_users 1025 out of \[1, 1024\]"),
            (dict(users=np.zeros((0, d), F32)), r"n_users 0 out of \[1, 1024\]"),
            (dict(users=us, topn=0), r"topn 0 out of \[1, 128\]"),
            (dict(users=us, topn=129), r"topn 129 out of \[1, 128\]"),
            (dict(users=us, embed_weight=0.0), "embed_weight 0: finite, not 0 and at most 4"),
            (dict(users=us, embed_weight=float("nan")), "embed_weight nan"),
            (dict(users=us, embed_weight=4.5), "embed_weight 4.5"),
            (dict(users=us, exclude=[[], list(range(65537)), []]), "user 1 excludes 65537 ids: at most 65536"),
        ]
        for kw, text in refusals:
            with pytest.raises(capi.Mi355Error, match=text) as err:
                tab.query_users(**kw)
            assert err.value.code == capi.ERR_INVALID_ARG, kw
        q = capi.EmbedBatchQuery(size=48, users=us.ctypes.data, n_users=3, topn=5, w_embed=1.0)
        idx = np.empty((3, 5), np.int64)
        res = capi.EmbedBatchResult(size=32, out_idx=idx.ctypes.data)
        assert L.mi355rec_embed_batch_query(tab._e, ctypes.byref(q), ctypes.byref(res)) == capi.OK   # out_score and out_count are optional
        assert idx[0].tolist() == bc.expected(table, us[0], "cosine", 1.0, 5)[0].tolist()
        for size in (0, 46, 52):
            q.size = size
            assert L.mi355rec_embed_batch_query(tab._e, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG
            assert b"embed batch query of size %d: not the end of a field of the 48 bytes" % size in L.mi355rec_embed_batch_last_error(tab._e)
        q.size, q.metric = 48, 2
        assert L.mi355rec_embed_batch_query(tab._e, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG
        info = capi.EmbedBatchInfo(size=40)
        assert L.mi355rec_embed_batch_info(tab._e, ctypes.byref(info)) == capi.ERR_INVALID_ARG
        served = tab.info()["users_served"]
        assert served == 3, "a refused call serves nobody"
        bc.check(tab, table, us, topn=40, metric="dot", embed_weight=2.0, what="after the refusals")
