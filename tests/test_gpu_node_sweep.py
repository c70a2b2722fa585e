"""The node handle over short and empty shards, on the MI355X (csrc/sharded.hip, csrc/node_state.hip.h): the request family's
twins on row-sharded placements of `devices=[0] * shards` whose shards are empty, hold one row, or hold fewer rows than topn
(tests/node_sweep_cases.py: the geometries, the catalogue, the request matrix and the oracles' expectations; the case
definitions themselves are checked on a host without a GPU by tests/test_node_sweep_cpu.py).

Per geometry: the matrix on the sharded handle as created and again after set_replica(ON) (the 8-bit copy built on demand: every
kernel's pre-filter at row_base != 0), on a single CosineEngine and on a replicated node handle, all four bit for bit equal and
equal to the oracle; row sets at whichever bit phase the geometry's shards start; side data dropped and set again; update_rows
across the shard edges.  Every call is a padded raw call: the count and the -1 / 0.0 past it are checked with it.  No tolerance."""
import time

import numpy as np
import pytest

from tests import node_sweep_cases as cases

pytestmark = pytest.mark.gpu
NARROW = [c for c in cases.CATALOGUES if c[:2] != cases.WIDE]
WIDE = [c for c in cases.CATALOGUES if c[:2] == cases.WIDE]


def _set_side_data(eng, cat):
    eng.set_labels(cat.labels)
    eng.set_priors(cat.priors)
    eng.set_groups(cat.groups)


def _run_all(eng, todo, what):
    """Every case on `eng`, each checked against the oracle; the results, for the comparison between handles."""
    got = []
    for c in todo:
        got.append(cases.run(eng, c))
        cases.check(c, got[-1], what)
    return got


def _equal(todo, a, b, what):
    for c, x, y in zip(todo, a, b):
        assert cases.same(x, y), f"{what}: {c.kind}: {c.what}"


def _sharded(cat):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    nd = NodeEngine(cat.feats, devices=[0] * cat.g, placement=capi.PLACEMENT_SHARDED)
    info = nd.info()
    assert info["n_shards"] == cat.g and info["rows"] == cat.n and info["shard_rows"] == cat.sizes, info
    return nd


def _matrix_on_every_handle(cat, todo, what):
    """Steps 1 to 3: the sharded handle as created and with the replica, the single handle, the replicated node.  Returns the
    seconds spent on the sharded handle."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    t0 = time.perf_counter()
    with _sharded(cat) as nd:
        _set_side_data(nd, cat)                                               # (with empty shards present)
        first = _run_all(nd, todo, f"{what} sharded")
        nd.set_replica(capi.REPLICA_ON)
        _equal(todo, first, _run_all(nd, todo, f"{what} sharded, replica on"), f"{what}: replica on against as created")
    spent = time.perf_counter() - t0
    with CosineEngine(cat.feats) as eng:
        _set_side_data(eng, cat)
        _equal(todo, first, _run_all(eng, todo, f"{what} single handle"), f"{what}: sharded against the single handle")
    with NodeEngine(cat.feats, devices=[0, 0], placement=capi.PLACEMENT_REPLICATED) as rep:
        _set_side_data(rep, cat)
        _equal(todo, first, _run_all(rep, todo, f"{what} replicated"), f"{what}: sharded against the replicated node")
    return spent


@pytest.mark.parametrize("n, g, variant", NARROW)
def test_request_matrix(engine_lib, n, g, variant):
    cat = cases.catalogue(n, g, variant)
    todo = cases.matrix(n, g, variant)
    spent = _matrix_on_every_handle(cat, todo, f"n={n} over {g} [{variant}]")
    print(f"n={n} over {g} [{variant}]: {len(todo)} cases, {spent:.2f} s on the sharded handle (twice the matrix)")


@pytest.mark.parametrize("n, g, variant", WIDE)
def test_request_matrix_on_64_shards(engine_lib, n, g, variant):
    """MI355REC_MAX_SHARDS shards of one or two rows: the plain cosine, bounded and any-of requests."""
    cat = cases.catalogue(n, g, variant)
    todo = cases.matrix(n, g, variant)
    assert {c.kind for c in todo} == set(cases.WIDE_KINDS)
    spent = _matrix_on_every_handle(cat, todo, f"n={n} over {g} [{variant}]")
    print(f"n={n} over {g} [{variant}]: {len(todo)} cases, {spent:.2f} s on the sharded handle (twice the matrix)")


@pytest.mark.parametrize("n, g, variant", NARROW)
def test_row_sets_side_data_and_updates(engine_lib, n, g, variant):
    """Steps 4 to 6 on one sharded handle."""
    import torch  # noqa: F401
    from spotify_recommender_amd import capi
    from tests.labels_oracle import check
    cat = cases.catalogue(n, g, variant)
    what = f"n={n} over {g} [{variant}]"
    short = cases.request_matrix(cat, short=True)
    with _sharded(cat) as nd:
        _set_side_data(nd, cat)
        # 4. row sets: every shard's slice starts at its own bit phase; a set that is one shard, one that is all but one shard
        for name, ids in cases.rowset_shapes(cat).items():
            for mode in ("seen", "only"):
                for kind, spec in (("cosine", dict(vecs=cat.std, topn=100)), ("anyof", dict(rows=cat.any_rows, topn=10)),
                                   ("bounded", dict(vecs=cat.std, metric="euclidean", bound=3e38, topn=1024))):
                    c = cases.expect(cat, cases.Case(kind, f"row set '{name}' as {mode}=", rowset=(ids, mode), **spec))
                    cases.check(c, cases.run(nd, c), what)
            # a set that grew by add() answers as one created whole: every shard's copy was refreshed
            if not ids:
                continue
            half = len(ids) // 2
            c = cases.expect(cat, cases.Case("cosine", f"row set '{name}' after add()", vecs=cat.std, rowset=(ids, "only"), topn=100))
            with nd.row_set(ids[:half]) as rs:
                rs.add(ids[half:] + ids[:1])
                assert rs.count == len(set(ids))
                check(nd.query_mean_topn(cat.std, 100, only=rs), c.want, f"{what} {c.what}")
                c = cases.expect(cat, cases.Case("cosine", f"row set '{name}' after add(), seen=", rows=cat.mrows, rowset=(ids, "seen"), topn=10))
                check(nd.query_playlist_topn(cat.mrows, 10, seen=rs), c.want, f"{what} {c.what}")
        # 5. side data dropped: the documented refusals; set again: the answers are back
        nd.set_labels(None)
        with pytest.raises(capi.Mi355Error, match="has no labels") as e:
            nd.query_mean_topn(cat.std, 10, labels=[cases.L_ALL])
        assert e.value.code == capi.ERR_INVALID_ARG
        nd.set_priors(None)
        with pytest.raises(capi.Mi355Error, match="has no priors") as e:
            nd.query_mean_topn(cat.std, 10, prior_weight=0.5)
        assert e.value.code == capi.ERR_INVALID_ARG
        nd.set_groups(None)
        with pytest.raises(capi.Mi355Error, match="has no groups") as e:
            nd.query_mean_topn_capped(cat.std, 10, 1)
        assert e.value.code == capi.ERR_INVALID_ARG
        c = cases.expect(cat, cases.Case("cosine", "plain, after the refusals", vecs=cat.std, topn=10))
        cases.check(c, cases.run(nd, c), what)                                # (the handle still answers)
        _set_side_data(nd, cat)
        _run_all(nd, short, f"{what} side data set again")
        # 6. update_rows across the shard edges, one shard left alone; norms, label-grouped copies, replica entries (the replica is
        # on from here) and the host copy of the groups follow
        nd.set_replica(capi.REPLICA_ON)
        _run_all(nd, short, f"{what} replica on")
        rows, new, after = cat.updated()
        nd.update_rows(rows, new)
        _run_all(nd, cases.request_matrix(after, short=True), f"{what} after update_rows")


def test_refusals_the_geometry_changes(engine_lib):
    """A row set of another node handle, a candidate id == n, a by-row member == n, update_rows([n]), an excluded id >= n: each
    ERR_INVALID_ARG, and the handle still answers.  (The single handle lets an excluded id >= n match nothing.)"""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import candidate_scores, query_anyof, with_candidates
    n, g = 13, 3
    cat = cases.catalogue(n, g)
    other = cases.catalogue(5, 8)
    plain = cases.expect(cat, cases.Case("cosine", "plain", vecs=cat.std, topn=10))
    with _sharded(cat) as nd, _sharded(other) as nd2:
        with nd2.row_set([0, 4]) as foreign:
            with pytest.raises(capi.Mi355Error, match="row set of another handle") as e:
                nd.query_mean_topn(cat.std, 10, seen=foreign)
            assert e.value.code == capi.ERR_INVALID_ARG
            with pytest.raises(capi.Mi355Error, match="row set of another handle") as e:
                query_anyof(nd, 10, members=cat.std, only=foreign)
            assert e.value.code == capi.ERR_INVALID_ARG
        for call in (lambda: with_candidates(nd, [0, n]).query_mean_topn(cat.std, 10),
                     lambda: candidate_scores(nd, [n, 0], queries=cat.std),
                     lambda: nd.query_playlist_topn([0, n], 10),
                     lambda: query_anyof(nd, 10, rows=[n]),
                     lambda: nd.update_rows([n], np.zeros((1, 12), np.float32)),
                     lambda: nd.query_mean_topn(cat.std, 10, exclude=cases.foreign_exclusions(cat)),
                     lambda: nd.row_set([0, n])):
            with pytest.raises(capi.Mi355Error) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARG, e.value
            cases.check(plain, cases.run(nd, plain), "after a refusal")
    with CosineEngine(cat.feats) as eng:
        c = cases.expect(cat, cases.Case("cosine", "ids >= n excluded", rows=cat.mrows, exclude=cases.foreign_exclusions(cat), topn=10))
        cases.check(c, cases.run(eng, c), "single handle")


@pytest.mark.parametrize("d", cases.EMBED_DIMS)
@pytest.mark.parametrize("n, g", cases.EMBED_GEOMETRIES)
def test_embedding_tables_on_short_shards(engine_lib, n, g, d):
    """Step 7: the fp32 embedding table made on the sharded node (mi355rec_embed_create_node), against tests/embed_oracle.py and
    equal to a table on the single engine."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from tests import embed_cases as ec
    from tests import embed_oracle as eo
    cat = cases.catalogue(n, g)
    table = np.random.default_rng([cases.SEED, n, g, d]).standard_normal((n, d), dtype=np.float32)
    for a, b in cat.pairs:
        table[b] = table[a]                                                   # (the audio rows of a pair are equal already)
    with _sharded(cat) as nd, EmbeddingTable(nd, table) as ntab, CosineEngine(cat.feats) as eng, EmbeddingTable(eng, table) as tab:
        for i, req in enumerate(cases.embed_requests(cat, d)):
            ec.check(ntab, cat.feats, table, req, f"n={n} over {g} d={d} request {i}")
            x, y = ntab.query(**req), tab.query(**req)
            assert x[0].tolist() == y[0].tolist() and np.array_equal(eo.bits(x[1]), eo.bits(y[1])), f"request {i}: node against single"
