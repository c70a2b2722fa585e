"""JACCARD REQUESTS on the MI355X (csrc/playlist.hip.h, "JACCARD": the kPlJaccard branch of playlist_row_key in
playlist_scan_kernel), through mi355rec_query_jaccard_request and its node-handle twin, bit for bit against
tests/jaccard_oracle.py: ids, similarity bits, counts and padding, no tolerances.  Sizes at the quad, the 2048-row tile,
kPlBoundRows, the 4096-row anchor table and several workgroups; on a handle that never built the 8-bit replica ("replica off")
and on one that did ("replica on": set_replica(ON) builds it on demand), as in tests/test_gpu_manhattan.py — there is no
pre-filter, so both take the chains on every row and must answer alike; one 1 000 003-row catalogue on which many workgroups
publish thresholds to each other."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.jaccard_oracle import check, expected_from_v, hostile_catalogue, mean_jaccard, request_call
from tests.labels_oracle import check as check_scores
from tests.playlist_labels_oracle import uniform_labels

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 4, 5, 2047, 2048, 2049, 4097, 65_537]
TOPNS = (1, 257, 1024)
N_BIG = 1_000_003


def _call(eng, **kw):
    from spotify_recommender_amd import capi
    rc, ids, sim = request_call(capi, eng._lib.mi355rec_query_jaccard_request, eng._h, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, sim


def _ext(rowset, mode):
    from spotify_recommender_amd import capi
    return capi.RequestExt(ctypes.sizeof(capi.RequestExt), mode, None, rowset._ptr())


def _engines(feats):
    """("replica off", engine) then ("replica on", engine), one alive at a time."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    with CosineEngine(feats, flags=capi.CREATE_NO_REPLICA) as eng:
        yield "replica off", eng
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        yield "replica on", eng


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    from spotify_recommender_amd import capi
    feats = oracle.mt19937_uniform(900 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    in_set = sorted({int(r) for r in rng.choice(n, size=max(1, n // 3), replace=False)})
    cases = []
    for k in (1, 3, 32):
        rows = [int(r) for r in rng.choice(n, size=k, replace=n < k)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = feats[3 if n > 3 else 0]                       # a member equal to rows of the catalogue: v = 1 and ties at K = 1
        cases.append((k, rows, vecs, mean_jaccard(feats, feats[rows]), mean_jaccard(feats, vecs)))
    results = {}
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        with eng.row_set(in_set) as rs:
            for k, rows, vecs, v_r, v_v in cases:
                for topn in TOPNS:
                    what = f"n={n} [{mode}] K={k} top-{topn}"
                    got = _call(eng, rows=rows, topn=topn)
                    check(got, expected_from_v(feats, v_r, rows, topn), what + " by row")
                    results.setdefault((k, topn, "row"), []).append(got)
                    got = _call(eng, members=vecs, topn=topn)
                    check(got, expected_from_v(feats, v_v, [], topn), what + " by value")
                    results.setdefault((k, topn, "value"), []).append(got)
                for rs_mode, only in ((capi.ROWSET_EXCLUDE, False), (capi.ROWSET_ONLY, True)):
                    check(_call(eng, members=vecs, exclude=[n - 1, 0, 0], where=WHERE, labels=WANTED, topn=257, ext=_ext(rs, rs_mode)),
                          expected_from_v(feats, v_v, [n - 1, 0], 257, WHERE, lab, WANTED, in_set, only),
                          f"n={n} [{mode}] K={k} composed, row set mode {rs_mode}")
                ids = _call(eng, rows=rows, topn=10, want_similarity=False)[0]   # out_similarity is optional
                assert ids.tolist() == expected_from_v(feats, v_r, rows, 10)[0].tolist()
    for key, (off, on) in results.items():                        # replica on and off: identical results
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [5, 4097, 70_001])
def test_hostile_rows_and_members(engine_lib, n):
    """NaN, +-inf, all-zero, 1e-30 and 1e30 rows, negative features, duplicates (v = 1, ties by row); members that are tiny, zero,
    huge, negative or not finite.  Rows that form no key are never returned: the count equals the admissible rows."""
    feats = hostile_catalogue(n)
    rng = np.random.default_rng([9, n])
    cases = []                                                     # (K, what, call arguments, excluded, (v, valid)): the oracle's values once
    for k in (1, 3, 32):
        rows = [0] + [int(r) for r in rng.choice(np.arange(1, n), size=k - 1, replace=n - 1 < k - 1)]   # hostile rows among them
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = feats[0]
        tiny = vecs.copy()
        tiny[k // 2] = np.float32(1e-30)
        zero = np.zeros((k, 12), np.float32)
        huge = vecs.copy()
        huge[k - 1] = np.float32(1e30)
        neg = vecs.copy()
        neg[k - 1, ::3] = -neg[k - 1, ::3]
        nan = vecs.copy()
        nan[k - 1, 5] = np.nan
        inf = vecs.copy()
        inf[k - 1, 2] = np.inf
        for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []), ("by row", dict(rows=rows), feats[rows], rows),
                                            ("tiny member", dict(members=tiny), tiny, []), ("zero members", dict(members=zero), zero, []),
                                            ("huge member", dict(members=huge), huge, []), ("negative member", dict(members=neg), neg, []),
                                            ("NaN member", dict(members=nan), nan, []), ("inf member", dict(members=inf), inf, [])):
            cases.append((k, what, kw, excluded, mean_jaccard(feats, members)))
    for mode, eng in _engines(feats):
        for k, what, kw, excluded, vv in cases:
            ok = vv[1].copy()
            ok[[e for e in excluded]] = False
            n_adm = int(ok.sum())
            for topn in sorted({1, 257, 1024, max(1, min(1024, n_adm)), min(1024, n_adm + 1)}):
                got = _call(eng, topn=topn, **kw)
                check(got, expected_from_v(feats, vv, excluded, topn), f"hostile n={n} [{mode}] K={k} {what} top-{topn}")
                assert got[0].size == min(topn, n_adm)
        ids, sim = _call(eng, members=feats[:1], topn=4)             # copies of the single member: exactly 1.0f, ties by row
        assert ids[0] == 0 and sim[0].view(np.uint32) == np.float32(1.0).view(np.uint32)
        if n > 40:
            assert ids.tolist() == [0, 8, 9, 10] and np.all(sim == np.float32(1.0))


@pytest.fixture(scope="module")
def big(engine_lib):
    """(feats, member rows, (v, valid) of every row): computed once, never modified."""
    feats = oracle.mt19937_uniform(2029, N_BIG)
    rows = [123_457, 700_001, 42]
    return feats, rows, mean_jaccard(feats, feats[rows])


def test_1m_rows_many_workgroups(big):
    """Top-100 of 1 000 003 uniform rows, K = 3: the oracle's answer with and without the replica, bit for bit alike.  There is
    no pre-filter: rows_exact grows by every row on both handles."""
    feats, rows, vv = big
    answers = []
    for mode, eng in _engines(feats):
        before = eng.playlist_counters()
        got = _call(eng, rows=rows, topn=100)
        after = eng.playlist_counters()
        exact = after["rows_exact"] - before["rows_exact"]
        print(f"[{mode}] rows_exact {exact} of {N_BIG}")
        check(got, expected_from_v(feats, vv, rows, 100), f"1 M rows [{mode}]")
        answers.append(got)
        assert after["queries"] - before["queries"] == 1
        assert exact == N_BIG, (mode, exact)
        got = _call(eng, rows=rows, exclude=[5, 6], where=WHERE, topn=100)              # the other shapes on many workgroups
        check(got, expected_from_v(feats, vv, rows + [5, 6], 100, WHERE), f"1 M rows [{mode}], by row, composed")
    check(answers[1], answers[0], "1 M rows: replica on against off")


def test_lanes_updates_rebuild_and_interleaving(engine_lib):
    """A lane gives its parent's bits; cosine, distance, any-of, Manhattan and bounded requests before and after a Jaccard request
    on the same handle (one staging buffer, one shared threshold word) return the bits they returned before it; after update_rows
    on 50 rows, and after rebuild_replica, the call equals a fresh handle's."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    n = 70_001
    feats = oracle.mt19937_uniform(26, n)
    rows = [7, 7_000, 69_999]
    vv = mean_jaccard(feats, feats[rows])
    want = expected_from_v(feats, vv, rows + [8, 9], 200, WHERE)

    def others(eng):
        return (eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE), eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE),
                engine.query_anyof(eng, 200, rows=rows, exclude=[8, 9], where=WHERE),
                engine.query_manhattan(eng, 200, rows=rows, exclude=[8, 9], where=WHERE),
                engine.query_bounded(eng, 200, 0.9, rows=rows, exclude=[8, 9], where=WHERE))

    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        before = others(eng)
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent")
        check(engine.query_jaccard(eng, 200, rows=rows, exclude=[8, 9], where=WHERE), want, "the Python function")
        after = others(eng)
        check_scores(after[0], before[0], "cosine by row after a Jaccard request")
        check_scores(after[1], before[1], "distance after a Jaccard request")
        for name, a, b in zip(("any-of", "Manhattan", "bounded"), after[2:], before[2:]):
            a, b = [np.asarray(x) for x in a], [np.asarray(x) for x in b]
            assert _same_bits(a, b), name + " after a Jaccard request"
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent, after the other requests")
        lane = eng.lane()
        try:
            check(_call(lane, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "lane")
            check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent, after the lane's call")
        finally:
            lane.close()
        # 50 rows change in place (some of them onto a member): the call answers as a fresh handle does
        rng = np.random.default_rng(73)
        changed_rows = np.sort(rng.choice(n, size=50, replace=False))
        changed = feats.copy()
        changed[changed_rows] = rng.random((changed_rows.size, 12), dtype=np.float32)
        changed[changed_rows[:20]] = feats[7] * np.float32(1.01)
        eng.update_rows(changed_rows, changed[changed_rows])
        vv2 = mean_jaccard(changed, changed[rows])
        want2 = expected_from_v(changed, vv2, rows + [8, 9], 200, WHERE)
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "after update_rows")
    with CosineEngine(changed) as fresh:   # (a handle that never had a lane: one that had cannot rebuild its replicas)
        fresh.set_replica(capi.REPLICA_ON)
        check(_call(fresh, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "a fresh handle")
        fresh.rebuild_replica()
        check(_call(fresh, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "after rebuild_replica")


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(13, n)
    feats[n - 5:] = feats[17]                                     # ties across the two shards
    lab = uniform_labels(n, 30, 9)
    rng = np.random.default_rng(10)
    seen = sorted({int(r) for r in rng.choice(n, size=n // 4, replace=False)})
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    with NodeEngine(feats, devices=[0, 0], placement=pl) as node, CosineEngine(feats) as eng:
        fn = node._lib.mi355rec_sharded_query_jaccard_request
        node.set_labels(lab)
        eng.set_labels(lab)
        for k in (1, 6, 32):
            rows = [17] + [int(r) for r in rng.choice(n, size=k - 1, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            vv = mean_jaccard(feats, feats[rows])
            for topn in (10, 1024):
                for kw, excluded in ((dict(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29]), rows + excl),
                                     (dict(members=feats[rows], exclude=excl), excl), (dict(rows=rows), rows)):
                    rc, ids, sim = request_call(capi, fn, node._h, topn=topn, **kw)
                    assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                    what = f"{placement} K={k} top-{topn} {sorted(kw)}"
                    check((ids, sim), _call(eng, topn=topn, **kw), what + " against the single handle")
                    check((ids, sim), expected_from_v(feats, vv, excluded, topn, kw.get("where"), lab, kw.get("labels")), what)
        # K = 1 by value with the member equal to row 17: rows 17 and n - 5 .. n - 1 tie at exactly 1.0f across the shard edge
        ids, sim = request_call(capi, fn, node._h, members=feats[17:18], topn=8)[1:]
        assert ids[:6].tolist() == [17, n - 5, n - 4, n - 3, n - 2, n - 1] and np.all(sim[:6] == np.float32(1.0)) and sim[6] < 1
        vv = mean_jaccard(feats, feats[[3, 4]])
        for kw, rs in ((dict(seen=seen), dict(rowset=seen, rowset_only=False)), (dict(only=seen), dict(rowset=seen, rowset_only=True))):
            got = engine.query_jaccard(node, 20, rows=[3, 4], **kw)
            check(got, engine.query_jaccard(eng, 20, rows=[3, 4], **kw), "the Python function, node against single handle")
            check(got, expected_from_v(feats, vv, [3, 4], 20, **rs), "the Python function with a row set")
        rc = request_call(capi, fn, node._h, members=feats[:2], flags=1)[0]
        assert rc == capi.ERR_INVALID_ARG and "must be 0" in node._lib.mi355rec_sharded_last_error(node._h).decode()


def test_one_shard_forwards(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 9_001
    feats = hostile_catalogue(n)
    rows = [0, 100, 9_000]
    vv = mean_jaccard(feats, feats[rows])
    with NodeEngine(feats, devices=[0], placement=capi.PLACEMENT_AUTO) as node:
        check(engine.query_jaccard(node, 50, rows=rows, exclude=[1], where=WHERE), expected_from_v(feats, vv, rows + [1], 50, WHERE), "one shard")


def test_the_cli_answers_as_the_cpu_backend_does(engine_lib, tmp_path):
    """One `--similarity jaccard` run on the GPU against the same run with no device visible (the CPU backend), each a fresh
    child process: the same recommendations and the same printed similarities."""
    from spotify_recommender_amd import build
    from tests.test_playlist_cpu import _write_csv
    build.build_shim()
    _write_csv(tmp_path / "songs.csv")
    pre = subprocess.run([str(build.BIN_CLI), "--preprocess", "songs.csv"], capture_output=True, text=True, cwd=tmp_path)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    ids = [l.split(",")[0] for l in (tmp_path / "songs.csv").read_text().splitlines()[1:]]
    args = [str(build.BIN_CLI), "--playlist", ",".join(ids[i] for i in (5, 70, 333)), "--similarity", "jaccard", "-n", "12", "--where", "energy=0.1:0.9"]
    gpu = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    cpu = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert gpu.returncode == 0 and cpu.returncode == 0, (gpu.stderr, cpu.stderr)
    tail = [p.stdout.split("Recommendations:", 1)[1] for p in (gpu, cpu)]
    assert tail[0] == tail[1] and len(re.findall(r"\(similarity ", tail[0])) == 12, tail
    assert "=== RECOMMENDATION MODE (Jaccard similarity) ===" in gpu.stdout
