"""FEATURE SCALES on the MI355X (csrc/playlist.hip.h, "FEATURE SCALES": the scaled branch of playlist_scan_kernel and the per-row
cut of its cosine pre-filter), through the four _scaled entry points, bit for bit against tests/scaled_oracle.py: ids, score and
distance bits, counts and padding, no tolerances.  Sizes at the quad, the 2048-row tile, kPlBoundRows, the 4096-row anchor table
and 33 workgroups that publish thresholds; on a handle without a replica (every row takes the chains) and on one with a replica
(the pre-filter of the cosine metric; scaled distance requests stay exact by design)."""
import numpy as np
import pytest

from oracle import oracle
from tests import distance_oracle, playlist_labels_oracle
from tests.playlist_labels_oracle import uniform_labels
from tests.scaled_oracle import (DROP3, GENERAL, SCALE_SETS, check, cosine_expected, cosine_scores, distance_expected, distance_m,
                                 request_call, scale)

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 4, 5, 257, 2047, 2048, 2049, 4097, 65_537]
TOPNS = (1, 10, 257, 1024)
N_BIG = 262_147
METRICS = ("cosine", "euclidean")
FN = {"cosine": "mi355rec_query_playlist_request_scaled", "euclidean": "mi355rec_query_distance_request_scaled"}


def _call(eng, metric, scales, **kw):
    from spotify_recommender_amd import capi
    rc, ids, val = request_call(capi, getattr(eng._lib, FN[metric]), eng._h, metric, scales, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, val


def _engines(feats):
    """("replica off", engine) then ("replica on", engine), one alive at a time (tests/test_gpu_distance.py)."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA if feats.shape[0] >= 65_536 else 0) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


def _oracle_values(metric, feats, members, a, weights=None):
    return distance_m(feats, members, a) if metric == "euclidean" else cosine_scores(feats, members, a, weights)


def _expected(metric, values, feats, excluded, topn, where=None, labels=None, wanted=None):
    fn = distance_expected if metric == "euclidean" else cosine_expected
    return fn(values, feats, excluded, topn, where, labels, wanted)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    feats = oracle.mt19937_uniform(900 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    cases = []
    for k in sorted({min(k, n) for k in (1, 3, 32)}):
        rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = feats[int(rng.integers(0, n))]
        signed = (rng.random(k, dtype=np.float32) + np.float32(0.1)) * np.where(np.arange(k) % 3 == 1, -1, 1).astype(np.float32)
        for sname, a in SCALE_SETS.items():
            for metric in METRICS:
                cases.append((k, rows, vecs, signed, sname, a, metric, _oracle_values(metric, feats, feats[rows], a),
                              _oracle_values(metric, feats, vecs, a),
                              _oracle_values(metric, feats, vecs, a, signed) if metric == "cosine" else None))
    results = {}
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        for k, rows, vecs, signed, sname, a, metric, v_r, v_v, v_w in cases:
            for topn in TOPNS:
                what = f"n={n} [{mode}] K={k} {sname} {metric} top-{topn}"
                got = _call(eng, metric, a, rows=rows, topn=topn)
                check(got, _expected(metric, v_r, feats, rows, topn), what + " by row")
                results.setdefault((k, sname, metric, topn), []).append(got)
                check(_call(eng, metric, a, members=vecs, topn=topn), _expected(metric, v_v, feats, [], topn), what + " by value")
                check(_call(eng, metric, a, members=vecs, exclude=[n - 1, 0, 0], where=WHERE, labels=WANTED, topn=topn),
                      _expected(metric, v_v, feats, [n - 1, 0], topn, WHERE, lab, WANTED), what + " composed")
            if metric == "cosine":
                check(_call(eng, metric, a, members=vecs, weights=signed, exclude=[0], where=WHERE, topn=10),
                      _expected(metric, v_w, feats, [0], 10, WHERE), f"n={n} [{mode}] K={k} {sname} signed weights")
    for key, (off, on) in results.items():                        # replica on and off: identical results
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [257, 4097, 65_537])
def test_second_handle_identity_and_null_scales(engine_lib, n):
    """A handle over scale(feats, a) answers the unscaled request for the members scale(q, a) with the ids and bits of the scaled
    request on the original handle; NULL scales and all ones are the unscaled entry point."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats = oracle.mt19937_uniform(31 + n % 7, n)
    rng = np.random.default_rng([3, n])
    rows = [int(r) for r in rng.choice(n, size=3, replace=False)]
    vecs = rng.random((3, 12), dtype=np.float32)
    plain = {"cosine": ("mi355rec_query_playlist_request", playlist_labels_oracle.request_call),
             "euclidean": ("mi355rec_query_distance_request", distance_oracle.request_call)}
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        for metric in METRICS:
            name, req = plain[metric]
            for kw in (dict(rows=rows), dict(members=vecs, exclude=[1, 2], where=WHERE)):
                unscaled = req(capi, getattr(eng._lib, name), eng._h, topn=100, **kw)[1:3]
                check(_call(eng, metric, None, topn=100, **kw), unscaled, f"{metric}: NULL scales")
                check(_call(eng, metric, np.ones(12, np.float32), topn=100, **kw), unscaled, f"{metric}: all ones")
        for sname, a in SCALE_SETS.items():
            with CosineEngine(scale(feats, a)) as other:
                other.set_replica(capi.REPLICA_ON)
                for metric in METRICS:
                    for topn in (10, 1024):
                        check(_call(eng, metric, a, rows=rows, topn=topn), _call(other, metric, None, rows=rows, topn=topn),
                              f"n={n} {sname} {metric} top-{topn}: second handle, by row")
                        check(_call(eng, metric, a, members=vecs, exclude=[5], topn=topn),
                              _call(other, metric, None, members=scale(vecs, a), exclude=[5], topn=topn),
                              f"n={n} {sname} {metric} top-{topn}: second handle, by value")


@pytest.mark.parametrize("n", [5, 257, 4097])
def test_hostile_rows_with_a_zero_scale_on_their_column(engine_lib, n):
    """NaN, +-inf (columns 2, 3, 4 of rows 2, 3, 4), all-zero, 1e-30 and 1e30 rows and duplicates: a zero scale on a column does
    not hide what it holds."""
    feats = distance_oracle.hostile_catalogue(n)
    a = GENERAL.copy()
    a[[2, 3, 4]] = 0
    rng = np.random.default_rng([9, n])
    for mode, eng in _engines(feats):
        for k in (1, 3, 32):
            rows = [0] + [int(r) for r in rng.choice(np.arange(1, n), size=min(k, n) - 1, replace=False)]
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            for scales in (a, DROP3, SCALE_SETS["EDGE"]):
                for metric in METRICS:
                    for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []), ("by row", dict(rows=rows), feats[rows], rows)):
                        values = _oracle_values(metric, feats, members, scales)
                        for topn in (1, 10, 1024):
                            check(_call(eng, metric, scales, topn=topn, **kw), _expected(metric, values, feats, excluded, topn),
                                  f"hostile n={n} [{mode}] K={k} {metric} {what} top-{topn}")
        ids, _ = _call(eng, "euclidean", a, members=feats[:1], topn=min(n, 1024))
        finite = int(np.isfinite(distance_m(feats, feats[:1], a)).sum())
        assert ids.size == min(finite, 1024) and not {2, 3, 4} & set(ids.tolist())      # the NaN and the +-inf rows are never listed


def test_a_row_sharded_node_equals_the_single_handle(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(10, n)
    feats[n - 5:] = feats[17]                                     # ties across the two shards
    lab = uniform_labels(n, 30, 9)
    rng = np.random.default_rng(10)
    node_fn = {"cosine": "mi355rec_sharded_query_playlist_request_scaled", "euclidean": "mi355rec_sharded_query_distance_request_scaled"}
    with NodeEngine(feats, devices=[0, 0], placement=capi.PLACEMENT_SHARDED) as node, CosineEngine(feats) as eng:
        node.set_labels(lab)
        eng.set_labels(lab)
        for k in (1, 6):
            rows = [17] + [int(r) for r in rng.choice(n, size=k - 1, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            for sname in ("DROP3", "GENERAL", "EDGE"):
                a = SCALE_SETS[sname]
                for metric in METRICS:
                    values = _oracle_values(metric, feats, feats[rows], a)
                    for kw, excluded in ((dict(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29]), rows + excl),
                                         (dict(members=feats[rows], exclude=excl), excl), (dict(rows=rows), rows)):
                        rc, ids, val = request_call(capi, getattr(node._lib, node_fn[metric]), node._h, metric, a, topn=100, **kw)
                        assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                        what = f"sharded K={k} {sname} {metric} {sorted(kw)}"
                        check((ids, val), _call(eng, metric, a, topn=100, **kw), what + " against the single handle")
                        check((ids, val), _expected(metric, values, feats, excluded, 100, kw.get("where"), lab, kw.get("labels")), what)
        check(node.query_playlist_topn([3, 4], 20, scales=DROP3), eng.query_playlist_topn([3, 4], 20, scales=DROP3), "the Python methods")
        check(node.query_nearest_rows_scaled([3, 4], 20, {"tempo": 2}), eng.query_nearest_rows_scaled([3, 4], 20, {"tempo": 2}), "nearest")
        rc = request_call(capi, getattr(node._lib, node_fn["cosine"]), node._h, "cosine", GENERAL, members=feats[:2], flags=capi.PQ_PRIOR)[0]
        assert rc == capi.ERR_INVALID_ARG and "with feature scales" in node._lib.mi355rec_sharded_last_error(node._h).decode()


def test_the_prefilter_works_and_scaled_distances_stay_exact(engine_lib):
    """Top-10 of 262 147 uniform rows, K = 1, DROP3: the oracle's answer, and rows_exact: at most n / 4 with the replica (the
    model gives under 1 % at the true threshold; the anchors' start is looser), exactly the rows read without it.  A scaled
    distance request computes every row's chains whatever the handle holds."""
    feats = oracle.mt19937_uniform(2027, N_BIG)
    q = feats[123_457].copy()
    sc = cosine_scores(feats, q[None, :], DROP3)
    m = distance_m(feats, q[None, :], DROP3)
    for mode, eng in _engines(feats):
        before = eng.playlist_counters()
        got = _call(eng, "cosine", DROP3, members=q, topn=10)
        after = eng.playlist_counters()
        exact = after["rows_exact"] - before["rows_exact"]
        print(f"[{mode}] scaled cosine: rows_exact {exact} of {N_BIG} ({100.0 * exact / N_BIG:.3f} %)")
        check(got, cosine_expected(sc, feats, [], 10), f"262 147 rows [{mode}]")
        assert after["queries"] - before["queries"] == 1
        if mode == "replica on":
            assert 0 < exact <= N_BIG // 4, exact
            check(_call(eng, "cosine", GENERAL, rows=[123_457], exclude=[5, 6], where=WHERE, topn=100),
                  cosine_expected(cosine_scores(feats, q[None, :], GENERAL), feats, [123_457, 5, 6], 100, WHERE), "by row, composed")
        else:
            assert exact == N_BIG, exact
        before = eng.playlist_counters()
        check(_call(eng, "euclidean", DROP3, members=q, topn=10), distance_expected(m, feats, [], 10), f"scaled distance [{mode}]")
        exact = eng.playlist_counters()["rows_exact"] - before["rows_exact"]
        print(f"[{mode}] scaled distance: rows_exact {exact} of {N_BIG}")
        assert exact == N_BIG, exact
