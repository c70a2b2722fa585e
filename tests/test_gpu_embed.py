"""EMBEDDING TABLES on the GPU (include/mi355rec_embed.h, csrc/embed.hip.h): embed_scan_kernel's answers bit for bit
against tests/embed_oracle.py at the sizes where the kernel can go wrong — the rows-per-wave-instruction edges of every
dim, one tile more or less, several workgroups, many per-workgroup lists in the merge — the parity hook for every row,
the CPU placement's recorded answers, a node handle of two virtual shards, updated audio rows, two tables on one handle.
Hostile means values, never addresses."""
import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_oracle as eo

pytestmark = pytest.mark.gpu
F32 = np.float32
DIMS = [16, 32, 64, 128]


def _tile_rows(d):
    """The scan's tile, asked of the library (a one-row table)."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    with CosineEngine(np.ones((1, 12), F32)) as eng, EmbeddingTable(eng, np.ones((1, d), F32)) as tab:
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
def test_scan_matches_the_oracle(d, group):
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    for n in _sizes(group, d):
        feats, table = ec.catalogue(n, d)
        with CosineEngine(feats) as eng, EmbeddingTable(eng, table) as tab:
            info = tab.info()
            assert (info["rows"], info["dim"], info["shards"]) == (n, d, 1) and info["device"] >= 0 and info["grid"] >= 1
            reqs = ec.requests(n, d)
            for i, req in enumerate(reqs):
                ec.check(tab, feats, table, req, f"n={n} d={d} request {i}")
            after = tab.info()
            with_audio = sum(1 for r in reqs if r.get("audio_weight", 0.0) != 0.0)
            assert after["queries"] == 2 * len(reqs) and after["scores_launches"] == 2 * with_audio   # none with w_audio == 0


def test_a_million_rows_many_lists():
    """1 000 003 rows at d = 16: every workgroup of the grid hands a list to the merge, top-10 and top-1024."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    n, d = 1_000_003, 16
    rng = np.random.default_rng(9)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    table[123_456] = table[7]
    feats[123_456] = feats[7]
    user = rng.standard_normal(d, dtype=F32)
    with CosineEngine(feats) as eng, EmbeddingTable(eng, table) as tab:
        assert tab.info()["grid"] > 64
        for topn in (10, 1024):
            req = dict(user=user, metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=7, topn=topn, exclude=[7, 7, n + 1])
            ec.check(tab, feats, table, req, f"top-{topn}", scores=topn == 10)
        ec.check(tab, feats, table, dict(rows=[5, 6, 7], metric="dot", embed_weight=1.0, topn=1024), "dot, top-1024", scores=False)


def test_gpu_equals_the_cpu_placement(golden_dir):
    """The answers the CPU placement gave for this catalogue (recorded by tests/test_embed_golden.py's case)."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from tests.test_embed_golden import GOLDEN_CASE, golden_answers
    n, d = GOLDEN_CASE
    feats, table = ec.catalogue(n, d)
    want = golden_answers(golden_dir)
    with CosineEngine(feats) as eng, EmbeddingTable(eng, table) as tab:
        for i, req in enumerate(ec.requests(n, d)):
            ids, sc = tab.query(**req)
            assert ids.tolist() == want[f"ids{i}"].tolist(), i
            assert np.array_equal(eo.bits(sc), want[f"score_bits{i}"]), i


def test_two_virtual_shards_equal_one_handle():
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.engine import NodeEngine
    n, d = 4099, 32
    feats, table = ec.catalogue(n, d)
    with NodeEngine(feats, devices=[0, 0]) as nd, EmbeddingTable(nd, table) as ntab, CosineEngine(feats) as eng, EmbeddingTable(eng, table) as tab:
        assert ntab.info()["shards"] == 2
        for i, req in enumerate(ec.requests(n, d)):
            ec.check(ntab, feats, table, req, f"two shards, request {i}")
            a, b = ntab.query(**req), tab.query(**req)
            assert a[0].tolist() == b[0].tolist() and np.array_equal(eo.bits(a[1]), eo.bits(b[1]))
        # member rows and the audio row on either side of the split
        req = dict(rows=[0, n - 1, n // 2, n // 2 - 1], metric="cosine", embed_weight=0.25, audio_weight=1.0, audio_row=n - 2, topn=100)
        ec.check(ntab, feats, table, req, "members on both shards")


def test_a_replicated_node_handle():
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.engine import NodeEngine
    n, d = 2050, 64
    feats, table = ec.catalogue(n, d)
    with NodeEngine(feats, devices=[0], placement=capi.PLACEMENT_REPLICATED) as nd, EmbeddingTable(nd, table) as tab:
        assert tab.info()["shards"] == 1
        ec.check(tab, feats, table, ec.requests(n, d)[1], "replicated")


def test_updated_rows_are_seen_by_the_next_call():
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    n, d = 70_001, 16
    feats, table = ec.catalogue(n, d)
    rng = np.random.default_rng(5)
    req = dict(rows=[4, 9, 100], metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=77, topn=50)
    with CosineEngine(feats) as eng, EmbeddingTable(eng, table) as tab:
        ec.check(tab, feats, table, req, "before the update")
        rows = [77, 0, n - 1, 500]
        new = rng.random((len(rows), 12), dtype=F32)
        feats[rows] = new
        eng.update_rows(rows, new)
        ec.check(tab, feats, table, req, "after the update")


def test_two_tables_on_one_handle():
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    n = 3001
    feats, t16 = ec.catalogue(n, 16)
    _, t128 = ec.catalogue(n, 128, seed=3)
    with CosineEngine(feats) as eng, EmbeddingTable(eng, t16) as a, EmbeddingTable(eng, t128) as b:
        for i in range(3):   # alternately: each table's buffers are its own
            ec.check(a, feats, t16, ec.requests(n, 16)[i], f"first table, request {i}")
            ec.check(b, feats, t128, ec.requests(n, 128)[i], f"second table, request {i}")
        # and the engine's own calls still answer between them
        from oracle import oracle
        idx, sc = eng.query_row_topn(5, 10)
        want = oracle.topn_canonical(oracle.scores(feats, feats[5]), 5, 10)
        assert idx.tolist() == want[0].tolist()


def test_a_shard_with_a_row_base():
    """A single handle that is one shard of a larger catalogue: ids are global, member and audio rows local."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    n, d, base = 1500, 32, 1_000_000
    feats, table = ec.catalogue(n, d)
    with CosineEngine(feats, row_base=base) as eng, EmbeddingTable(eng, table) as tab:
        req = dict(rows=[3, 4, 5], metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=10, topn=40, exclude=[base + 7, 7, base + n])
        ec.check(tab, feats, table, req, "row_base", row_base=base)
