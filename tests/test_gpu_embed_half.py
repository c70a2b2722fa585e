"""HALF-PRECISION EMBEDDING TABLES on the GPU (include/mi355rec_embed_half.h, csrc/embed_half.hip.h):
embed_half_scan_kernel's answers, both storages, bit for bit against tests/embed_oracle.py over the WIDENED table — v and
c of every row through the parity hook and the top-N — at the sizes where the kernel can go wrong: the
rows-per-wave-instruction edges of every dim (32 / 16 / 8 / 4), one tile more or less (1024 rows at d = 16: the candidate
list's widest append), several workgroups, a full grid of lists in the merge (no workgroup sees more than two tiles
here; many tiles per workgroup, repeated compaction and a list at its last slot are tests/test_gpu_embed_steady.py's); rows
that only half storage makes hostile (the largest fp16, the first value that rounds to inf, the smallest fp16 subnormal —
a flushing kernel scores it as zero — and 3e38); the fp32 library on the widened table; the CPU placement's recorded
answers; a row base; updated audio rows; two tables of different storage on one handle.  Hostile means values, never
addresses."""
import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_half_cases as hc
from tests import embed_oracle as eo

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = [16, 32, 64, 128]


def _tile_rows(d, storage):
    """The scan's tile, asked of the library (a one-row table)."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    with CosineEngine(np.ones((1, 12), F32)) as eng, HalfEmbeddingTable(eng, np.ones((1, d), F32), storage=storage) as tab:
        return tab.info()["tile_rows"]


def _sizes(group, d, storage):
    if group == "edges":
        return [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33]
    if group == "tile":
        t = _tile_rows(d, storage)
        assert t == 2048 // (d // 8)
        return [t - 1, t, t + 1]
    return [4097] if group == "blocks" else [65537]


@pytest.mark.parametrize("storage", hc.STORAGES)
@pytest.mark.parametrize("group", ["edges", "tile", "blocks", "many"])
@pytest.mark.parametrize("d", DIMS)
def test_scan_matches_the_oracle_over_the_widened_table(d, group, storage):
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    code = capi.EMBED_HALF_FP16 if storage == "fp16" else capi.EMBED_HALF_BF16
    for n in _sizes(group, d, storage):
        feats, words = hc.catalogue(n, d, storage)
        with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, hc.as_given(words, storage)) as tab:
            info = tab.info()
            assert (info["rows"], info["dim"], info["shards"], info["storage"]) == (n, d, 1, code) and info["device"] >= 0 and info["grid"] >= 1
            assert np.array_equal(tab.words(), words)   # attached as it is
            wide = tab.widened()
            if n >= 17:   # the subnormal row is there, exactly
                assert np.all(wide[14] == F32(2.0 ** -24))
            reqs = ec.requests(n, d)
            for i, req in enumerate(reqs):
                ec.check(tab, feats, wide, req, f"{storage} n={n} d={d} request {i}")
            after = tab.info()
            with_audio = sum(1 for r in reqs if r.get("audio_weight", 0.0) != 0.0)
            assert after["queries"] == 2 * len(reqs) and after["scores_launches"] == 2 * with_audio   # none with w_audio == 0


@pytest.mark.parametrize("storage", hc.STORAGES)
def test_a_million_rows_many_lists(storage):
    """1 000 003 rows at d = 16 (977 tiles: the grid is full): every workgroup hands a list to the merge, top-10 and top-1024."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    n, d = 1_000_003, 16
    rng = np.random.default_rng(9)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    table[123_456] = table[7]
    feats[123_456] = feats[7]
    user = rng.standard_normal(d, dtype=F32)
    with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, table, storage=storage) as tab:
        assert tab.info()["grid"] > 64 and tab.info()["tile_rows"] == 1024
        wide = tab.widened()
        for topn in (10, 1024):
            req = dict(user=user, metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=7, topn=topn, exclude=[7, 7, n + 1])
            ec.check(tab, feats, wide, req, f"top-{topn}", scores=topn == 10)
        ec.check(tab, feats, wide, dict(rows=[5, 6, 7], metric="dot", embed_weight=1.0, topn=1024), "dot, top-1024", scores=False)


@pytest.mark.parametrize("storage", hc.STORAGES)
@pytest.mark.parametrize("n,d", [(4099, 32), (3001, 128)])
def test_the_half_library_equals_the_fp32_library_on_the_widened_table(n, d, storage):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    feats, words = hc.catalogue(n, d, storage)
    with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, hc.as_given(words, storage)) as tab:
        with EmbeddingTable(eng, tab.widened()) as full:
            assert tab.info()["device_bytes"] < full.info()["device_bytes"]
            for i, req in enumerate(ec.requests(n, d)):
                a, b = tab.query(**req), full.query(**req)
                assert a[0].tolist() == b[0].tolist(), (storage, i)
                assert np.array_equal(eo.bits(a[1]), eo.bits(b[1])), (storage, i)


@pytest.mark.parametrize("storage", hc.STORAGES)
def test_gpu_equals_the_cpu_placement(golden_dir, storage):
    """The answers the fp32 library's CPU placement gave for the widened table (tests/test_embed_half_golden.py's case)."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    from tests.test_embed_half_golden import GOLDEN_CASE, golden_answers, golden_words
    n, d = GOLDEN_CASE
    feats, words = golden_words(storage)
    want = golden_answers(golden_dir)
    with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, hc.as_given(words, storage)) as tab:
        for i, req in enumerate(ec.requests(n, d)):
            ids, sc = tab.query(**req)
            assert ids.tolist() == want[f"{storage}_ids{i}"].tolist(), i
            assert np.array_equal(eo.bits(sc), want[f"{storage}_score_bits{i}"]), i


@pytest.mark.parametrize("storage", hc.STORAGES)
def test_a_shard_with_a_row_base(storage):
    """A single handle that is one shard of a larger catalogue: ids are global, member and audio rows local."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    n, d, base = 1500, 32, 1_000_000
    feats, words = hc.catalogue(n, d, storage)
    with CosineEngine(feats, row_base=base) as eng, HalfEmbeddingTable(eng, hc.as_given(words, storage)) as tab:
        req = dict(rows=[3, 4, 5], metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=10, topn=40, exclude=[base + 7, 7, base + n])
        ec.check(tab, feats, tab.widened(), req, "row_base", row_base=base)


@pytest.mark.parametrize("storage", hc.STORAGES)
def test_updated_rows_are_seen_by_the_next_call(storage):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    n, d = 70_001, 16
    feats, words = hc.catalogue(n, d, storage)
    rng = np.random.default_rng(5)
    req = dict(rows=[4, 9, 100], metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=77, topn=50)
    with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, hc.as_given(words, storage)) as tab:
        wide = tab.widened()
        ec.check(tab, feats, wide, req, "before the update")
        rows = [77, 0, n - 1, 500]
        new = rng.random((len(rows), 12), dtype=F32)
        feats[rows] = new
        eng.update_rows(rows, new)
        ec.check(tab, feats, wide, req, "after the update")


def test_two_tables_of_different_storage_on_one_handle():
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    n = 3001
    feats, w16 = hc.catalogue(n, 16, "fp16")
    _, w128 = hc.catalogue(n, 128, "bf16", seed=3)
    with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, hc.as_given(w16, "fp16")) as a, HalfEmbeddingTable(eng, hc.as_given(w128, "bf16")) as b:
        for i in range(3):   # alternately: each table's buffers are its own
            ec.check(a, feats, a.widened(), ec.requests(n, 16)[i], f"fp16 table, request {i}")
            ec.check(b, feats, b.widened(), ec.requests(n, 128)[i], f"bf16 table, request {i}")
        # and the engine's own calls still answer between them
        from oracle import oracle
        idx, sc = eng.query_row_topn(5, 10)
        want = oracle.topn_canonical(oracle.scores(feats, feats[5]), 5, 10)
        assert idx.tolist() == want[0].tolist()


def test_a_narrow_float32_table_is_rounded_and_zero_padded():
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable, to_storage, widen
    n = 300
    feats, table = ec.catalogue(n, 32)
    with CosineEngine(feats) as eng, HalfEmbeddingTable(eng, table[:, :20], storage="bf16") as tab:
        assert (tab.user_dim, tab.dim, tab.storage) == (20, 32, 1)
        wide = np.zeros((n, 32), F32)
        wide[:, :20] = widen(to_storage(table[:, :20], "bf16"), "bf16")
        assert ec.same_floats(tab.widened(), wide)
        req = dict(user=table[7, :20], metric="cosine", embed_weight=1.0, audio_weight=0.5, audio_row=3, topn=25)
        full = dict(req, user=np.concatenate([table[7, :20], np.zeros(12, F32)]))
        v, c, ids, sc = ec.expected(feats, wide, full)
        gi, gs = tab.query(**req)
        assert gi.tolist() == ids.tolist() and np.array_equal(eo.bits(gs), eo.bits(sc))


def test_refusals_leave_the_table_answering():
    import ctypes
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    n, d = 40, 16
    feats, words = hc.catalogue(n, d, "fp16")
    L = capi.embed_half_lib()

    def raw(w, rows, dim, storage, eng):
        e = ctypes.c_void_p()
        rc = L.mi355rec_embed_half_create(eng._h, w.ctypes.data_as(ctypes.c_void_p), rows, dim, storage, ctypes.byref(e))
        assert rc == capi.ERR_INVALID_ARG and not e
        return L.mi355rec_embed_half_last_error(None)

    with CosineEngine(feats) as eng:
        assert b"embedding dim 24: 16, 32, 64 or 128" in raw(np.zeros((n, 24), np.uint16), n, 24, 0, eng)
        assert b"table of 39 rows for a handle of 40 rows" in raw(words, n - 1, d, 0, eng)
        assert b"storage 2: MI355REC_EMBED_HALF_FP16 (0) or MI355REC_EMBED_HALF_BF16 (1)" in raw(words, n, d, 2, eng)
        e = ctypes.c_void_p()
        assert L.mi355rec_embed_half_create(eng._h, None, n, d, 0, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        with pytest.raises(capi.Mi355Error, match="table of 41 rows for a handle of 40 rows"):
            HalfEmbeddingTable(eng, np.zeros((n + 1, d), np.float16))
        with HalfEmbeddingTable(eng, hc.as_given(words, "fp16")) as tab:
            user = tab.widened()[2].copy()
            for kw, text in [(dict(rows=list(range(33))), "33 member rows: 1 to 32 are supported"),
                             (dict(user=user, topn=1025), r"topn 1025 out of \[1, 1024\]"),
                             (dict(user=user, embed_weight=0.0), "embed_weight 0: finite, not 0 and at most 4"),
                             (dict(user=user, audio_weight=1.0), "needs audio by value or a valid audio_row, got row -1"),
                             (dict(user=user, exclude=list(range(1025))), r"n_exclude 1025 out of \[0, 1024\]"),
                             (dict(rows=[n]), "Invalid song index: 40")]:
                with pytest.raises(capi.Mi355Error, match=text) as err:
                    tab.query(**kw)
                assert err.value.code == capi.ERR_INVALID_ARG, kw
            info = capi.EmbedHalfInfo(size=56)
            assert L.mi355rec_embed_half_info(tab._e, ctypes.byref(info)) == capi.ERR_INVALID_ARG
            assert b"embed half info of size 56: this library writes 64 bytes" in L.mi355rec_embed_half_last_error(tab._e)
            ec.check(tab, feats, tab.widened(), ec.requests(n, d)[1], "after the refusals")
