"""DIVERSIFIED TOP-N on the MI355X: MMR re-ranking of a relevance pool by mmr_rerank_kernel (csrc/diverse.hip.h), checked
against the oracle (tests/diverse_oracle.py): identical ids, bit-equal relevance, bit-equal mmr.  Two catalogues that keep
an 8-bit replica (1 M uniform rows; 1 M rows in 300 contiguous clusters), each through six routes that must give ONE answer:
a CosineEngine with the replica on and off, a lane, a node handle row-sharded over virtual shards {0, 0, 0} (the pool gathered
by mi355rec_fetch_rows and re-ranked by value), a replicated node handle {0, 0}.  Also the identities, mi355rec_fetch_rows
against the matrix, duplicates and ties, a filter that leaves fewer rows than asked, the counters and the argument errors."""
import numpy as np
import pytest

from oracle import oracle
from tests.diverse_oracle import LAMBDAS, WHERE, check3, expected, expected_rows, pools, rerank, run_variant, variant_pool, variants
from tests.labels_oracle import check

pytestmark = pytest.mark.gpu

N = 1_000_000


def _uniform():
    feats = oracle.mt19937_uniform(78, N)
    feats[10:14] = 0.0                  # zero rows
    feats[100:110] = feats[99]          # copies of row 99
    return np.ascontiguousarray(feats)


def _clustered():
    from spotify_recommender_amd.synth import clustered_catalogue
    return np.ascontiguousarray(clustered_catalogue(N, 0.03, seed=4242 + 300, clusters=300, contiguous=True, ramp=False, device="cpu").numpy())


@pytest.fixture(scope="module", params=["uniform", "clustered"])
def routes(request, engine_lib):
    """{route name: engine object} over one catalogue, and the catalogue."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = _uniform() if request.param == "uniform" else _clustered()
    with CosineEngine(feats) as eng, NodeEngine(feats, devices=[0, 0, 0], placement=capi.PLACEMENT_SHARDED) as sharded, \
            NodeEngine(feats, devices=[0, 0], placement=capi.PLACEMENT_REPLICATED) as replicated:
        lane = eng.lane()
        try:
            yield {"engine": eng, "lane": lane, "sharded {0,0,0}": sharded, "replicated {0,0}": replicated}, feats
        finally:
            lane.close()


def _every_route(rt, call, want, what):
    from spotify_recommender_amd import capi
    eng = rt["engine"]
    for name, obj in rt.items():
        check3(call(obj), want, f"{what} [{name}]")
    for mode, name in ((capi.REPLICA_OFF, "engine, replica off"), (capi.REPLICA_ON, "engine, replica on")):
        eng.set_replica(mode)
        try:
            check3(call(eng), want, f"{what} [{name}]")
        finally:
            eng.set_replica(capi.REPLICA_ON)


@pytest.mark.parametrize("k", [1, 2, 7, 32])
def test_diverse_queries_match_the_oracle_on_every_route(routes, k):
    rt, feats = routes
    for topn in (1, 10, 256):
        rng = np.random.default_rng(k * 1000 + topn)
        for v in variants(rng, feats, k):
            pidx, prel = variant_pool(feats, v, 1024)          # (a smaller pool is a prefix of it: canonical order)
            for pool in pools(topn):
                for lam in LAMBDAS:
                    _every_route(rt, lambda e: run_variant(e, feats, v, lam, pool, topn), rerank(feats, pidx[:pool], prel[:pool], lam, topn),
                                 f"k={k} top-{topn} pool {pool} lambda {lam} {v[0]}")


@pytest.mark.parametrize("k", [1, 7])
def test_identities_lambda_one_and_pool_equal_topn(routes, k):
    rt, feats = routes
    rng = np.random.default_rng(90 + k)
    rows = rng.choice(N, size=k, replace=False)
    w = rng.normal(0.0, 1.0, k).astype(np.float32)
    excl = rng.integers(0, N, size=50)
    for name, e in rt.items():
        for topn in (1, 10, 256):
            plain = e.query_playlist_topn(rows, topn, excl, where=WHERE, weights=w)
            for pool in pools(topn):
                idx, rel, mmr = e.query_playlist_topn_diverse(rows, topn, 1.0, pool, exclude=excl, where=WHERE, weights=w, return_mmr=True)
                check((idx, rel), plain, f"lambda 1, top-{topn} pool {pool} [{name}]")
                assert np.array_equal(mmr.view(np.uint32), rel.view(np.uint32)), name
            for lam in (0.0, 0.3, 0.7):
                idx, rel = e.query_playlist_topn_diverse(rows, topn, lam, topn, exclude=excl, where=WHERE, weights=w)
                order, want = np.argsort(idx), np.argsort(plain[0])
                assert idx[order].tolist() == plain[0][want].tolist(), f"pool == topn is a permutation (lambda {lam}, top-{topn}) [{name}]"
                assert np.array_equal(rel[order].view(np.uint32), plain[1][want].view(np.uint32)), name
                assert idx[0] == plain[0][0]


def test_fetch_rows_against_the_matrix(routes):
    rt, feats = routes
    eng = rt["engine"]
    rng = np.random.default_rng(5)
    for count in (1, 63, 64, 65, 1000, 1024, 1025, 3000):
        rows = rng.integers(0, N, size=count)                  # any order, duplicates allowed
        rows[count // 2] = rows[0]
        assert np.array_equal(eng.fetch_rows(rows).view(np.uint32), feats[rows].view(np.uint32)), count
    assert np.array_equal(eng.fetch_rows([N - 1, 0, N - 1, 0]), feats[[N - 1, 0, N - 1, 0]])
    assert eng.fetch_rows([]).shape == (0, 12)
    from spotify_recommender_amd import capi
    for bad in ([N], [-1], [0, N]):
        with pytest.raises(capi.Mi355Error) as e:
            eng.fetch_rows(bad)
        assert e.value.code == capi.ERR_INVALID_ARG
    assert np.array_equal(rt["lane"].fetch_rows([7, 7, 3]), feats[[7, 7, 3]])


def test_duplicates_ties_and_a_tight_filter(routes):
    rt, feats = routes
    near = feats[99] + np.float32(0.01) * feats[1099]           # next to row 99 (and, on the uniform catalogue, its ten copies)
    zero = np.zeros((1, 12), np.float32)
    tight = {0: (0.0, 0.001), 1: (0.0, 0.2)}
    for lam in (0.3, 0.7):
        _every_route(rt, lambda e: e.query_mean_topn_diverse(near[None, :], 40, lam, 60, return_mmr=True),
                     expected(feats, near[None, :], None, [], None, lam, 60, 40), f"copies, lambda {lam}")
        _every_route(rt, lambda e: e.query_mean_topn_diverse(zero, 30, lam, 64, return_mmr=True), expected(feats, zero, None, [], None, lam, 64, 30),
                     f"a zero query, lambda {lam}")
        want = expected_rows(feats, [7, 8], None, [], tight, lam, 1024, 256)
        _every_route(rt, lambda e: e.query_playlist_topn_diverse([7, 8], 256, lam, 1024, where=tight, return_mmr=True), want,
                     f"a tight filter, lambda {lam}")
    print(f"tight filter: {want[0].size} admissible rows")


def test_counters_advance(routes):
    rt, feats = routes
    eng = rt["engine"]
    before = eng.playlist_counters()["queries"]
    eng.query_playlist_topn_diverse([5, 6], 10, 0.5)
    eng.query_mean_topn_diverse(feats[[5, 6]], 10, 0.5, 10)
    assert eng.playlist_counters()["queries"] == before + 2


def test_argument_errors(routes):
    from spotify_recommender_amd import capi
    rt, feats = routes
    ones2 = np.ones((2, 12), np.float32)
    for name, e in rt.items():
        bad_calls = [
            lambda: e.query_playlist_topn_diverse([1, 2], 10, np.nan, 40),
            lambda: e.query_playlist_topn_diverse([1, 2], 10, -0.1, 40),
            lambda: e.query_mean_topn_diverse(ones2, 10, 1.5, 40),
            lambda: e.query_playlist_topn_diverse([1, 2], 10, 0.5, 9),
            lambda: e.query_mean_topn_diverse(ones2, 10, 0.5, 1025),
            lambda: e.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, weights=[0.0, 0.0]),
            lambda: e.query_playlist_topn_diverse([1], 10, 0.5, 40, where={1: (0.9, 0.1)}),
            lambda: e.query_playlist_topn_diverse(list(range(33)), 10, 0.5, 40),
            lambda: e.query_playlist_topn_diverse([N], 10, 0.5, 40),
        ]
        for i, call in enumerate(bad_calls):
            with pytest.raises(capi.Mi355Error) as err:
                call()
            assert err.value.code == capi.ERR_INVALID_ARG and str(err.value), (name, i)
        check3(e.query_playlist_topn_diverse([1, 2], 10, 0.5, 40, weights=[1.0, -0.5], return_mmr=True),
               expected_rows(feats, [1, 2], [1.0, -0.5], [], None, 0.5, 40, 10), f"after errors [{name}]")
