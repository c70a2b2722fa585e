"""ROW PRIORS on the MI355X (csrc/playlist.hip.h, "ROW PRIORS": the per-row cut of playlist_scan_kernel's pre-filter and
v = fl(s + fl(beta p)) in its exact chains), through the C-ABI's mi355rec_query_playlist_request, bit for bit against the
composed oracle (tests/prior_oracle.py): ids, score bits, counts and padding, no tolerances.  Sizes around every boundary of the
kernel (the tail quad and the priors' padding, the 2048-row tile, the 4096-row anchor table, the replica's 65 536 rows) without
a replica (every row exact) and with one (the pre-filter), and a 262 144-row catalogue on which several workgroups scan eight
tiles or more each, so thresholds published by one are taken by the others.

Which copy a playlist call scans: the 8-bit replica whenever the handle HAS one, so "replica off" below is a handle that never
built one (fewer than 65 536 rows, or CREATE_NO_REPLICA) and "replica on" one that did (set_replica(ON) builds it on demand)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.diverse_oracle import check3
from tests.labels_oracle import check
from tests.playlist_labels_oracle import uniform_labels
from tests.prior_oracle import expected_diverse, expected_prior, prior_kinds, request_call, scores_of

pytestmark = pytest.mark.gpu

N_BIG = 262_144
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
SIZES = [1, 3, 4, 5, 2047, 2048, 2049, 4095, 4096, 4097, 65_537]
TOPNS = (1, 10, 256, 257, 1024)   # (the anchor bound is off above 256)
BETAS = (0.25, 1.0, -0.5, 4.0)


def _capi():
    from spotify_recommender_amd import capi
    return capi


def _call(eng, **kw):
    capi = _capi()
    rc, ids, sc, mmr, p = request_call(capi, eng._lib.mi355rec_query_playlist_request, eng._h, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, sc, mmr, p


def _engines(feats):
    """("replica off", engine) then ("replica on", engine), one alive at a time."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA if feats.shape[0] >= 65_536 else 0) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    feats = oracle.mt19937_uniform(500 + n % 89, n)
    rng = np.random.default_rng(n)
    p = prior_kinds(rng, n)["signed"]
    p[n - 1] = np.float32(1.0)                                  # the last row (the tail quad) carries the largest prior
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    cases = []
    for k in sorted({min(k, n) for k in (1, 3, 32)}):
        rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
        vecs = rng.random((k, 12), dtype=np.float32)
        w = np.where(np.arange(k) % 3 == 2, -0.5, 1.0).astype(np.float32)   # dislikes from K = 3 on
        cases.append((k, rows, vecs, w, scores_of(feats, feats[rows]), scores_of(feats, vecs), scores_of(feats, vecs, w)))
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        eng.set_priors(p)
        for k, rows, vecs, w, s_r, s_v, s_w in cases:
            for topn in TOPNS:
                beta = BETAS[(topn + k) % len(BETAS)]
                what = f"n={n} [{mode}] K={k} top-{topn} beta {beta}"
                check(_call(eng, rows=rows, topn=topn, prior_weight=beta)[:2], expected_prior(s_r, p, beta, feats, lab, None, rows, topn),
                      what + " by row")
                check(_call(eng, members=vecs, topn=topn, prior_weight=beta)[:2], expected_prior(s_v, p, beta, feats, lab, None, [], topn),
                      what + " by value")
                check(_call(eng, members=vecs, weights=w, exclude=[n - 1, 0], where=WHERE, labels=[0, 2, 5], topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_w, p, beta, feats, lab, [0, 2, 5], [n - 1, 0], topn, WHERE), what + " composed")
            # the flag with beta = 0 is the call without the flag
            check(_call(eng, rows=rows, topn=10, prior_weight=0.0)[:2], _call(eng, rows=rows, topn=10)[:2], f"n={n} [{mode}] K={k} beta 0")
        eng.set_priors(np.zeros(n, np.float32))                  # all priors +0.0f is no prior
        k, rows = cases[-1][0], cases[-1][1]
        check(_call(eng, rows=rows, topn=10, prior_weight=4.0)[:2], _call(eng, rows=rows, topn=10)[:2], f"n={n} [{mode}] zero priors")


@pytest.fixture(scope="module")
def big(engine_lib):
    """(engine, feats, {kind: priors}, member rows, {k: scores of every row}): computed once, never modified."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = oracle.mt19937_uniform(2025, N_BIG)
    pri = prior_kinds(np.random.default_rng(5), N_BIG)
    rows = np.random.default_rng(12).choice(N_BIG, size=32, replace=False)
    scores = {k: scores_of(feats, feats[rows[:k]]) for k in (1, 3, 32)}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield eng, feats, pri, rows, scores


@pytest.mark.parametrize("kind", ["uniform", "skewed", "signed"])
@pytest.mark.parametrize("k", [1, 3, 32])
def test_262k_matches_the_oracle_and_the_prefilter_runs(big, kind, k):
    eng, feats, pri, rows, scores = big
    p = pri[kind]
    eng.set_priors(p)
    members = [int(r) for r in rows[:k]]
    for beta in BETAS:
        for topn in TOPNS:
            before = eng.playlist_counters()["rows_exact"]
            got = _call(eng, rows=members, topn=topn, prior_weight=beta)
            exact = eng.playlist_counters()["rows_exact"] - before
            check(got[:2], expected_prior(scores[k], p, beta, feats, None, None, members, topn), f"{kind} K={k} beta {beta} top-{topn}")
            print(f"{kind} K={k} beta {beta} top-{topn}: rows_exact {exact} ({100.0 * exact / N_BIG:.2f} %)")
            # the pre-filter ran.  (Above 256 the anchor bound is off: every workgroup takes its whole first tile, an eighth of
            # its rows, and the next few at a weak threshold; only the count is printed there.)
            assert exact > 0 and (topn > 256 or exact < N_BIG // 2), (kind, k, beta, topn, exact)
    # a call without the flag afterwards: unchanged
    check(_call(eng, rows=members, topn=100)[:2], expected_prior(scores[k], p, None, feats, None, None, members, 100), "no prior after")


def test_262k_compositions(big):
    eng, feats, pri, rows, scores = big
    p = pri["skewed"]
    lab = uniform_labels(N_BIG, 114, 7)
    groups = (np.arange(N_BIG) % 5).astype(np.int32)
    eng.set_priors(p)
    eng.set_labels(lab)
    eng.set_groups(groups)
    try:
        rng = np.random.default_rng(2)
        members = [int(r) for r in rows[:10]]
        w = np.where(np.arange(10) % 3 == 2, -0.5, 1.0).astype(np.float32)
        s_w = scores_of(feats, feats[members], w)
        wanted = [5, 60, 61, 113]
        for beta in (1.0, -0.5):
            top = expected_prior(s_w, p, beta, feats, lab, wanted, members, 200)[0]
            excl = np.concatenate([top[::2], rng.integers(0, N_BIG, size=200)]).tolist()
            for topn in (10, 1024):
                what = f"beta {beta} top-{topn}"
                check(_call(eng, rows=members, weights=w, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_w, p, beta, feats, lab, None, members, topn), what + " weights")
                check(_call(eng, rows=members, weights=w, exclude=excl, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_w, p, beta, feats, lab, None, members + excl, topn), what + " excluded")
                check(_call(eng, rows=members, weights=w, where=WHERE, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_w, p, beta, feats, lab, None, members, topn, WHERE), what + " filter")
                check(_call(eng, rows=members, weights=w, labels=wanted, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_w, p, beta, feats, lab, wanted, members, topn), what + " labels")
                check(_call(eng, members=feats[members], weights=w, exclude=excl, where=WHERE, labels=wanted, topn=topn, prior_weight=beta)[:2],
                      expected_prior(s_w, p, beta, feats, lab, wanted, excl, topn, WHERE), what + " all together, by value")
            for pool in (64, 1024):                              # the pool is the top-`pool` by v, rel = v
                pl = expected_prior(s_w, p, beta, feats, lab, wanted, members + excl, pool, WHERE)
                kw = dict(rows=members, weights=w, exclude=excl, where=WHERE, labels=wanted, topn=10, pool=pool, prior_weight=beta)
                for lam in (0.5, 1.0):
                    check3(_call(eng, lam=lam, **kw)[:3], expected_diverse(pl, feats, lam, 10), f"beta {beta} diverse {pool} {lam}")
                    got = _call(eng, lam=lam, max_per_group=1, **kw)
                    check3(got[:3], expected_diverse(pl, feats, lam, 10, groups, 1), f"beta {beta} capped {pool} {lam}")
                    assert got[3] == pl[0].size
        # count below topn: the padding behind it is checked by request_call
        few = np.flatnonzero(lab == 7)[:3]
        lab2 = lab.copy()
        lab2[lab2 == 7] = 8
        lab2[few] = 7
        eng.set_labels(lab2)
        ids, sc, _, _ = _call(eng, rows=members, labels=[7], topn=10, prior_weight=1.0)
        check((ids, sc), expected_prior(scores_of(feats, feats[members]), p, 1.0, feats, lab2, [7], members, 10), "three rows")
        assert ids.size == 3
    finally:
        eng.set_groups(None)
        eng.set_labels(None)


def test_massive_ties(big):
    eng, feats, pri, rows, scores = big
    members = [int(r) for r in rows[:3]]
    for name, p in (("two-valued", (np.arange(N_BIG) % 2).astype(np.float32)), ("all-equal", np.full(N_BIG, 0.5, np.float32))):
        eng.set_priors(p)
        for beta in (4.0, -4.0):
            for topn in (10, 1024):
                check(_call(eng, rows=members, topn=topn, prior_weight=beta)[:2],
                      expected_prior(scores[3], p, beta, feats, None, None, members, topn), f"{name} beta {beta} top-{topn}")


def test_hostile_rows(engine_lib):
    n = 70_001
    rng = np.random.default_rng(6)
    feats = rng.random((n, 12), dtype=np.float32)
    vals = [np.nan, np.inf, -np.inf, 1e-42, 3e19, -3e19]
    spots = rng.choice(n, size=600, replace=False)
    for i, r in enumerate(spots):
        feats[r, rng.integers(0, 12)] = vals[i % len(vals)]
    feats[spots[:50]] = 0.0                                      # zero rows
    feats[n - 1] = np.float32(3e19)
    p = prior_kinds(rng, n)["signed"]
    p[spots[::2]] = np.float32(1.0)                              # the hostile rows carry the largest priors
    good = np.setdiff1d(np.arange(n), spots)[:40]
    for mode, eng in _engines(feats):
        eng.set_priors(p)
        for k in (1, 3, 32):
            members = [int(r) for r in good[:k]]
            s = scores_of(feats, feats[members])
            for beta, topn in ((4.0, 1024), (0.25, 257), (-0.5, 10), (1.0, 1)):
                check(_call(eng, rows=members, topn=topn, prior_weight=beta)[:2], expected_prior(s, p, beta, feats, None, None, members, topn),
                      f"hostile [{mode}] K={k} beta {beta} top-{topn}")
        hostile = [int(spots[60]), int(spots[61]), int(good[0])]   # hostile members: the pre-filter is off for the query
        s = scores_of(feats, feats[hostile])
        check(_call(eng, rows=hostile, topn=100, prior_weight=1.0)[:2], expected_prior(s, p, 1.0, feats, None, None, hostile, 100),
              f"hostile members [{mode}]")


def test_lanes_share_the_priors(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    n = 70_001
    feats = oracle.mt19937_uniform(19, n)
    rng = np.random.default_rng(19)
    pri = prior_kinds(rng, n)
    rows = [7, 7_000, 69_999]
    s = scores_of(feats, feats[rows])
    with CosineEngine(feats) as eng:
        with pytest.raises(capi.Mi355Error, match="has no priors"):
            eng.query_playlist_topn(rows, 10, prior_weight=1.0)
        eng.set_priors(pri["uniform"])
        eng.set_priors(pri["skewed"])                            # a second call replaces
        want = expected_prior(s, pri["skewed"], 1.0, feats, None, None, rows + [8, 9], 200, WHERE)
        check(eng.query_playlist_topn(rows, 200, [8, 9], where=WHERE, prior_weight=1.0), want, "parent")
        lane = eng.lane()
        try:
            check(lane.query_playlist_topn(rows, 200, [8, 9], where=WHERE, prior_weight=1.0), want, "lane")
            for h in (eng, lane):                                # a handle that has lanes refuses the call
                with pytest.raises(capi.Mi355Error, match="has lanes"):
                    h.set_priors(pri["uniform"])
            check(lane.query_playlist_topn(rows, 200, [8, 9], where=WHERE, prior_weight=1.0), want, "lane, after the refusal")
        finally:
            lane.close()
        bad = pri["uniform"].copy()
        bad[123] = np.float32(1.5)
        with pytest.raises(capi.Mi355Error, match="row 123"):
            eng.set_priors(bad)
        check(eng.query_playlist_topn(rows, 200, [8, 9], where=WHERE, prior_weight=1.0), want, "a failed call leaves the priors")
        with pytest.raises(capi.Mi355Error, match="priors for a handle of"):
            eng.set_priors(pri["uniform"][:-1])
        for beta in (float("nan"), 5.0):
            rc = request_call(capi, eng._lib.mi355rec_query_playlist_request, eng._h, rows=rows, prior_weight=beta)[0]
            assert rc == capi.ERR_INVALID_ARG and "prior_weight" in eng._lib.mi355rec_last_error(eng._h).decode()
        rc = request_call(capi, eng._lib.mi355rec_query_playlist_request, eng._h, rows=rows, prior_weight=1.0, size=84)[0]
        assert rc == capi.ERR_INVALID_ARG and "MI355REC_PQ_PRIOR" in eng._lib.mi355rec_last_error(eng._h).decode()
        rc = request_call(capi, eng._lib.mi355rec_query_playlist_request, eng._h, rows=rows, flags=8)[0]
        assert rc == capi.ERR_INVALID_ARG and "unknown flags" in eng._lib.mi355rec_last_error(eng._h).decode()
        eng.set_priors(None)
        with pytest.raises(capi.Mi355Error, match="has no priors"):
            eng.query_playlist_topn(rows, 10, prior_weight=1.0)
        assert ctypes.sizeof(capi.PlaylistQuery) == 88


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(10, n)
    lab = uniform_labels(n, 30, 9)
    groups = (np.arange(n) % 4).astype(np.int32)
    rng = np.random.default_rng(10)
    p = prior_kinds(rng, n)["skewed"]
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    fn = None
    with NodeEngine(feats, devices=[0, 0], placement=pl) as node:
        fn = node._lib.mi355rec_sharded_query_playlist_request

        def call(**kw):
            rc, ids, sc, mmr, pr = request_call(capi, fn, node._h, **kw)
            assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
            return ids, sc, mmr, pr

        with pytest.raises(capi.Mi355Error, match="has no priors"):
            node.query_playlist_topn([1, 2], 10, prior_weight=1.0)
        node.set_labels(lab)
        node.set_groups(groups)
        node.set_priors(p)
        for k in (1, 6, 32):
            rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            s = scores_of(feats, feats[rows])
            for beta in (0.25, -0.5, 4.0):
                for topn in (10, 1024):
                    what = f"{placement} K={k} beta {beta} top-{topn}"
                    check(call(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29], topn=topn, prior_weight=beta)[:2],
                          expected_prior(s, p, beta, feats, lab, [0, 7, 29], rows + excl, topn, WHERE), what + " by row")
                    check(call(members=feats[rows], exclude=excl, topn=topn, prior_weight=beta)[:2],
                          expected_prior(s, p, beta, feats, lab, None, excl, topn), what + " by value")
                pool = expected_prior(s, p, beta, feats, lab, None, rows + excl, 64, WHERE)
                got = call(rows=rows, exclude=excl, where=WHERE, topn=10, lam=0.5, pool=64, max_per_group=1, prior_weight=beta)
                check3(got[:3], expected_diverse(pool, feats, 0.5, 10, groups, 1), f"{placement} K={k} beta {beta} capped")
                assert got[3] == 64
            check(call(rows=rows, topn=50, prior_weight=0.0)[:2], call(rows=rows, topn=50)[:2], f"{placement} K={k} beta 0")
        bad = p.copy()
        bad[n - 2] = np.nan
        with pytest.raises(capi.Mi355Error, match=f"row {n - 2}"):
            node.set_priors(bad)
        check(node.query_playlist_topn([3, 4], 20, prior_weight=1.0),
              expected_prior(scores_of(feats, feats[[3, 4]]), p, 1.0, feats, lab, None, [3, 4], 20), "a failed call leaves the priors")
        node.set_priors(None)
        with pytest.raises(capi.Mi355Error, match="has no priors"):
            node.query_playlist_topn([1, 2], 10, prior_weight=1.0)
