"""GROUP CAPS on the MI355X: "at most M per group" inside mmr_rerank_kernel (csrc/diverse.hip.h), both its serial loop
(lambda < 1) and its loop-free path (lambda == 1), checked against the oracle (tests/capped_oracle.py): identical ids,
bit-equal relevance, bit-equal mmr, the count and P'.  One catalogue of 70 001 rows (the smallest that keeps an 8-bit
replica; odd, so the last quad is partial) with a few zero rows and ten copies of one row, through six routes that must give
ONE answer: a CosineEngine with the replica on and off, a lane made after set_groups, a node handle row-sharded over virtual
shards {0, 0, 0} (the pool straddles the shards; its groups are passed by value), a replicated node handle {0, 0}."""
import contextlib

import numpy as np
import pytest

from oracle import oracle
from tests.capped_oracle import (WHERE, cap_holds, check3, check4, in_order_capped, layouts, pools, rerank_capped, run_variant, variant_pool,
                                 variants)
from tests.weighted_oracle import expected as pool_expected

pytestmark = pytest.mark.gpu

N = 70_001
COPIES_GROUP = 5_000_000


@pytest.fixture(scope="module")
def base(engine_lib):
    """The three handles that own rows, the catalogue and the group layouts."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = oracle.mt19937_uniform(78, N)
    feats[10:14] = 0.0                  # zero rows
    feats[100:110] = feats[99]          # copies of row 99
    feats = np.ascontiguousarray(feats)
    lay = layouts(N)
    shared = lay["row // 3"].copy()
    shared[99:110] = COPIES_GROUP
    lay["the copies share one group"] = shared
    with CosineEngine(feats) as eng, NodeEngine(feats, devices=[0, 0, 0], placement=capi.PLACEMENT_SHARDED) as sharded, \
            NodeEngine(feats, devices=[0, 0], placement=capi.PLACEMENT_REPLICATED) as replicated:
        yield {"engine": eng, "sharded {0,0,0}": sharded, "replicated {0,0}": replicated}, feats, lay


@contextlib.contextmanager
def grouped(owners, groups):
    """Every route with `groups` set: the owners, and a lane of the engine made AFTER set_groups (it shares them)."""
    for o in owners.values():
        o.set_groups(groups)
    lane = owners["engine"].lane()
    try:
        yield dict(owners, lane=lane)
    finally:
        lane.close()
        for o in owners.values():
            o.set_groups(None)


def _every_route(rt, call, want3, pool_rows, what):
    from spotify_recommender_amd import capi
    eng = rt["engine"]
    for name, obj in rt.items():
        check4(call(obj), want3, pool_rows, f"{what} [{name}]")
    for mode, name in ((capi.REPLICA_OFF, "engine, replica off"), (capi.REPLICA_ON, "engine, replica on")):
        eng.set_replica(mode)
        try:
            check4(call(eng), want3, pool_rows, f"{what} [{name}]")
        finally:
            eng.set_replica(capi.REPLICA_ON)


LAYOUTS = ("row % 7", "row // 3", "all -1", "a third -1", "near 2^31", "the copies share one group")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_capped_queries_match_the_oracle_on_every_route(base, layout):
    owners, feats, lay = base
    g = lay[layout]
    short = 0
    with grouped(owners, g) as rt:
        for k, pick in ((1, 0), (7, 3), (32, 2)):               # by row; by value, signed weights, excluded, filtered; dislikes
            for topn in (1, 10, 256, 1024):
                rng = np.random.default_rng(k * 1000 + topn)
                v = list(variants(rng, feats, k))[pick]
                pidx, prel = variant_pool(feats, v, 1024)      # (a smaller pool is a prefix of it: canonical order)
                for pool in pools(topn):
                    for lam in (0.0, 0.7, 1.0):
                        for m in (1, 3):
                            want = rerank_capped(feats, pidx[:pool], prel[:pool], g, lam, m, topn)
                            what = f"{layout} k={k} top-{topn} pool {pool} lambda {lam} M {m} {v[0]}"
                            assert cap_holds(want[0], g, m)
                            _every_route(rt, lambda e: run_variant(e, v, lam, pool, m, topn), want, min(pool, pidx.size), what)
                            short += want[0].size < min(topn, pool)
    if layout == "row % 7":
        assert short > 0, "the cap must bind somewhere: count < topn"


def test_the_copies_in_one_group(base):
    """Ten copies of row 99 (and row 99) share a group: a query next to them has them at the head of the pool."""
    owners, feats, lay = base
    g = lay["the copies share one group"]
    near = (feats[99] + np.float32(0.01) * feats[1099])[None, :]
    pidx, prel = pool_expected(feats, near, [1.0], [], 64, None)
    assert set(range(99, 110)) <= set(pidx.tolist())
    with grouped(owners, g) as rt:
        for lam in (0.0, 0.7, 1.0):
            for m in (1, 3):
                want = rerank_capped(feats, pidx, prel, g, lam, m, 40)
                copies = sum(99 <= i <= 109 for i in want[0].tolist())          # (lambda < 1 pushes the copies back by itself)
                assert copies == m if lam == 1.0 else 1 <= copies <= m
                _every_route(rt, lambda e: e.query_mean_topn_capped(near, 40, m, lam, 64, return_mmr=True, return_pool_rows=True), want, 64,
                             f"copies, lambda {lam}, M {m}")
        # a zero query: every rel is +0.0, ties go by pool position
        zero = np.zeros((1, 12), np.float32)
        zp = pool_expected(feats, zero, [1.0], [], 64, None)
        for lam in (0.5, 1.0):
            _every_route(rt, lambda e: e.query_mean_topn_capped(zero, 30, 1, lam, 64, return_mmr=True, return_pool_rows=True),
                         rerank_capped(feats, *zp, g, lam, 1, 30), 64, f"a zero query, lambda {lam}")


def test_boundary_sizes(base):
    owners, feats, lay = base
    rows = [7, 8, 60_000]
    members, excluded = feats[rows], rows
    g = lay["row // 3"].copy()
    g[::2] = (np.arange(N)[::2] % 11).astype(np.int32)          # half the rows in eleven big groups, the rest in small ones
    tight = {0: (0.0, 0.005), 1: (0.0, 0.5)}
    one = np.zeros(N, np.int32)
    full, _ = pool_expected(feats, members, np.ones(3, np.float32), excluded, 1024, None), None
    tp = pool_expected(feats, members, np.ones(3, np.float32), excluded, 1024, tight)
    assert 20 < tp[0].size < 1024
    print(f"tight filter: {tp[0].size} admissible rows")
    with grouped(owners, g) as rt:
        for lam in (1.0, 0.5):
            # pool sizes at the wave edges
            for pool in (63, 64, 65, 1024):
                for topn, m in ((30, 2), (pool, 2), (pool, 1)):
                    want = rerank_capped(feats, full[0][:pool], full[1][:pool], g, lam, m, topn)
                    _every_route(rt, lambda e: e.query_playlist_topn_capped(rows, topn, m, lam, pool, return_mmr=True, return_pool_rows=True),
                                 want, pool, f"pool {pool} top-{topn} M {m} lambda {lam}")
            # P' < pool through a tight filter
            for topn, m in ((10, 1), (256, 2)):
                want = rerank_capped(feats, tp[0], tp[1], g, lam, m, topn)
                _every_route(rt, lambda e: e.query_playlist_topn_capped(rows, topn, m, lam, 1024, where=tight, return_mmr=True,
                                                                        return_pool_rows=True), want, tp[0].size, f"tight filter top-{topn} lambda {lam}")
            # max_per_group = topn is the diverse call, on every route
            for name, e in rt.items():
                for topn, pool in ((10, 40), (64, 65), (256, 1024)):
                    check3(e.query_playlist_topn_capped(rows, topn, topn, lam, pool, return_mmr=True),
                           e.query_playlist_topn_diverse(rows, topn, lam, pool, return_mmr=True), f"M = topn = {topn}, lambda {lam} [{name}]")
    # every row in one group, M = 1: one pick
    with grouped(owners, one) as rt:
        for lam in (1.0, 0.5):
            for pool in (1, 64, 1024):
                want = (full[0][:1], full[1][:1], (np.float32(lam) * full[1][:1]).astype(np.float32))
                check3(rerank_capped(feats, full[0][:pool], full[1][:pool], one, lam, 1, min(pool, 10)), want, "the oracle itself")
                _every_route(rt, lambda e: e.query_playlist_topn_capped(rows, min(pool, 10), 1, lam, pool, return_mmr=True, return_pool_rows=True),
                             want, pool, f"one group, pool {pool}, lambda {lam}")


def test_set_groups_again_drop_lanes_counters_and_errors(base):
    from spotify_recommender_amd import capi
    owners, feats, lay = base
    eng = owners["engine"]
    rows = [5, 6]
    pidx, prel = pool_expected(feats, feats[rows], np.ones(2, np.float32), rows, 80, None)

    def refused(call, word=None):
        with pytest.raises(capi.Mi355Error) as err:
            call()
        assert err.value.code == capi.ERR_INVALID_ARG and str(err.value)
        if word:
            assert word in str(err.value), str(err.value)

    # a handle without groups refuses, on every route
    for name, e in owners.items():
        refused(lambda: e.query_playlist_topn_capped(rows, 10, 2), "groups")
    with grouped(owners, lay["row % 7"]) as rt:
        for lam in (0.5, 1.0):
            _every_route(rt, lambda e: e.query_playlist_topn_capped(rows, 10, 1, lam, 80, return_mmr=True, return_pool_rows=True),
                         rerank_capped(feats, pidx, prel, lay["row % 7"], lam, 1, 10), 80, f"row % 7, lambda {lam}")
        # the engine has a lane now: set_groups is refused, on the engine and on the lane, and nothing changes
        refused(lambda: eng.set_groups(lay["row // 3"]), "lanes")
        refused(lambda: rt["lane"].set_groups(lay["row // 3"]), "lanes")
        refused(lambda: eng.set_groups(None), "lanes")
        check3(eng.query_playlist_topn_capped(rows, 10, 1, 0.5, 80, return_mmr=True), rerank_capped(feats, pidx, prel, lay["row % 7"], 0.5, 1, 10),
               "after the refused set_groups")
        # counters advance
        before = eng.playlist_counters()["queries"]
        eng.query_playlist_topn_capped(rows, 10, 2)
        eng.query_mean_topn_capped(feats[rows], 10, 2, 0.5, 10)
        assert eng.playlist_counters()["queries"] == before + 2
        # the argument errors, then a good call
        ones2 = np.ones((2, 12), np.float32)
        bad = lay["row // 3"].copy()
        bad[N - 1] = -2
        for name, e in rt.items():
            for call in (lambda: e.query_playlist_topn_capped(rows, 10, 0), lambda: e.query_mean_topn_capped(ones2, 10, -1),
                         lambda: e.query_playlist_topn_capped(rows, 10, 2, np.nan, 40), lambda: e.query_mean_topn_capped(ones2, 10, 2, 1.5, 40),
                         lambda: e.query_playlist_topn_capped(rows, 10, 2, 0.5, 9), lambda: e.query_mean_topn_capped(ones2, 10, 2, 0.5, 1025),
                         lambda: e.query_playlist_topn_capped(rows, 10, 2, 0.5, 40, weights=[0.0, 0.0]),
                         lambda: e.query_playlist_topn_capped([N], 10, 2, 0.5, 40)):
                refused(call)
            if name not in ("engine", "lane"):
                refused(lambda: e.set_groups(bad))
                refused(lambda: e.set_groups(bad[:-1]))
            check4(e.query_playlist_topn_capped(rows, 10, 1, 0.5, 80, return_mmr=True, return_pool_rows=True),
                   rerank_capped(feats, pidx, prel, lay["row % 7"], 0.5, 1, 10), 80, f"after the errors [{name}]")
    # (the lane is gone) set_groups again with other groups changes the answer accordingly, without dropping in between
    for o in owners.values():
        o.set_groups(lay["row % 7"])
    try:
        for layout in ("row // 3", "near 2^31"):
            for name, o in owners.items():
                refused(lambda: o.set_groups(bad[:-1]))                          # a failure leaves the previous groups in place
                o.set_groups(lay[layout])
                for lam in (0.5, 1.0):
                    check4(o.query_playlist_topn_capped(rows, 10, 1, lam, 80, return_mmr=True, return_pool_rows=True),
                           rerank_capped(feats, pidx, prel, lay[layout], lam, 1, 10), 80, f"replaced by {layout} [{name}]")
        assert in_order_capped(pidx, prel, lay["row // 3"], 1, 10)[0].tolist() != in_order_capped(pidx, prel, lay["near 2^31"], 1, 10)[0].tolist()
    finally:
        for o in owners.values():
            o.set_groups(None)
    for name, e in owners.items():
        refused(lambda: e.query_playlist_topn_capped(rows, 10, 2), "groups")
