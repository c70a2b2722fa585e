"""MANHATTAN REQUESTS on the MI355X (csrc/anyof.hip.h: manhattan_scan_kernel; csrc/playlist_cut.hip.h,
"MANHATTAN": its per-member cut over the 8-bit replica and the stored norms), through mi355rec_query_manhattan_request and its
node-handle twin, bit for bit against tests/manhattan_oracle.py: ids, distance bits, counts and padding, no tolerances.  Sizes at
the quad, the 2048-row tile, kPlBoundRows, the 4096-row anchor table and several workgroups; without a replica (every row takes
the chains) and with one (the pre-filter); one 1 000 003-row catalogue on which many workgroups publish thresholds to each other.

Which copy the scan reads: the 8-bit replica whenever the handle HAS one, so "replica off" is a handle that never built one and
"replica on" one that did (set_replica(ON) builds it on demand), as in tests/test_gpu_distance.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import check as check_scores
from tests.manhattan_oracle import check, expected_from_m, hostile_catalogue, mean_l1, request_call
from tests.playlist_labels_oracle import uniform_labels

pytestmark = pytest.mark.gpu

WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
SIZES = [1, 4, 5, 257, 2047, 2048, 2049, 4097, 65_537]
TOPNS = (1, 10, 256, 257, 1024)
N_BIG = 1_000_003


def _call(eng, **kw):
    from spotify_recommender_amd import capi
    rc, ids, dist = request_call(capi, eng._lib.mi355rec_query_manhattan_request, eng._h, **kw)
    assert rc == capi.OK, eng._lib.mi355rec_last_error(eng._h)
    return ids, dist


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


def _member_cases(rng, feats):
    """[(k, rows, vecs, m by row, m by value)]: the oracle's values once per set of members."""
    n = feats.shape[0]
    out = []
    for k in (1, 3, 32):
        rows = [int(r) for r in rng.choice(n, size=k, replace=n < k)]
        vecs = rng.random((k, 12), dtype=np.float32)
        vecs[0] = np.nan_to_num(feats[int(rng.integers(0, n))], nan=0.5, posinf=1.0, neginf=-1.0)
        out.append((k, rows, vecs, mean_l1(feats, feats[rows]), mean_l1(feats, vecs)))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engine_lib, n):
    from spotify_recommender_amd import capi
    feats = oracle.mt19937_uniform(800 + n % 89, n)
    if n > 40:
        feats[n - 1] = feats[3]                                  # duplicates: ties by row, in the tail quad too
        feats[n // 2] = feats[3]
    rng = np.random.default_rng(n)
    lab = uniform_labels(n, 6, n, unlabelled=0.1)
    in_set = sorted({int(r) for r in rng.choice(n, size=max(1, n // 3), replace=False)})
    cases = _member_cases(rng, feats)
    results = {}
    for mode, eng in _engines(feats):
        eng.set_labels(lab)
        with eng.row_set(in_set) as rs:
            for k, rows, vecs, m_r, m_v in cases:
                for topn in TOPNS:
                    what = f"n={n} [{mode}] K={k} top-{topn}"
                    got = _call(eng, rows=rows, topn=topn)
                    check(got, expected_from_m(feats, m_r, rows, topn), what + " by row")
                    results.setdefault((k, topn), []).append(got)
                    check(_call(eng, members=vecs, topn=topn), expected_from_m(feats, m_v, [], topn), what + " by value")
                    for rs_mode, only in ((capi.ROWSET_EXCLUDE, False), (capi.ROWSET_ONLY, True)):
                        check(_call(eng, members=vecs, exclude=[n - 1, 0, 0], where=WHERE, labels=WANTED, topn=topn, ext=_ext(rs, rs_mode)),
                              expected_from_m(feats, m_v, [n - 1, 0], topn, WHERE, lab, WANTED, in_set, only),
                              what + f" composed, row set mode {rs_mode}")
                check(_call(eng, rows=rows, topn=10, labels=WANTED), expected_from_m(feats, m_r, rows, 10, None, lab, WANTED), "labels")
                check(_call(eng, rows=rows, topn=10, where=WHERE), expected_from_m(feats, m_r, rows, 10, WHERE), "filter")
                check(_call(eng, rows=rows, topn=10, exclude=[1, 2, n - 1]), expected_from_m(feats, m_r, rows + [1, 2, n - 1], 10), "exclusion")
                ids = _call(eng, rows=rows, topn=10, want_distance=False)[0]   # out_distance is optional
                assert ids.tolist() == expected_from_m(feats, m_r, rows, 10)[0].tolist()
    for key, (off, on) in results.items():                        # replica on and off: identical results
        check(on, off, f"n={n} {key}: replica on against off")


@pytest.mark.parametrize("n", [5, 257, 4097, 70_001])
def test_hostile_rows_and_members(engine_lib, n):
    """NaN, +-inf, all-zero, 1e-30 and 1e30 rows, duplicates (m = 0 as +0.0, ties by row); members that are tiny, zero, huge
    or not finite (the cut is off for the last two).  Rows whose m is not finite form no key: the count says so."""
    feats = hostile_catalogue(n)
    rng = np.random.default_rng([9, n])
    for mode, eng in _engines(feats):
        for k in (1, 3, 32):
            rows = [0] + [int(r) for r in rng.choice(np.arange(1, n), size=k - 1, replace=n - 1 < k - 1)]   # hostile rows among them
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            tiny = vecs.copy()
            tiny[k // 2] = np.float32(1e-30)
            zero = np.zeros((k, 12), np.float32)
            huge = vecs.copy()
            huge[k - 1] = np.float32(1e30)
            nan = vecs.copy()
            nan[k - 1, 5] = np.nan
            for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []), ("by row", dict(rows=rows), feats[rows], rows),
                                                ("tiny member", dict(members=tiny), tiny, []), ("zero members", dict(members=zero), zero, []),
                                                ("huge member", dict(members=huge), huge, []), ("NaN member", dict(members=nan), nan, [])):
                m = mean_l1(feats, members)
                ok = np.isfinite(m)
                ok[[e for e in excluded]] = False
                n_adm = int(ok.sum())
                for topn in sorted({1, 10, 257, 1024, max(1, min(1024, n_adm)), min(1024, n_adm + 1)}):
                    got = _call(eng, topn=topn, **kw)
                    check(got, expected_from_m(feats, m, excluded, topn), f"hostile n={n} [{mode}] K={k} {what} top-{topn}")
                    assert got[0].size == min(topn, n_adm)
        ids, dist = _call(eng, members=feats[:1], topn=4)             # copies of the member: m = 0 is +0.0, ties by row
        assert ids[0] == 0 and not dist[:1].view(np.uint32).any()


@pytest.fixture(scope="module")
def big(engine_lib):
    """(feats, member rows, m of every row): computed once, never modified."""
    feats = oracle.mt19937_uniform(2027, N_BIG)
    rows = [123_457, 700_001, 42]
    return feats, rows, mean_l1(feats, feats[rows])


def test_1m_rows_many_workgroups_and_the_prefilter_works(big):
    """Top-100 of 1 000 003 uniform rows, K = 3: the oracle's answer with and without the replica, bit for bit alike, and
    rows_exact: every row without the replica, fewer than the row count with it (the share is printed)."""
    feats, rows, m = big
    answers = []
    for mode, eng in _engines(feats):
        before = eng.playlist_counters()
        got = _call(eng, rows=rows, topn=100)
        after = eng.playlist_counters()
        exact = after["rows_exact"] - before["rows_exact"]
        print(f"[{mode}] rows_exact {exact} of {N_BIG} ({100.0 * exact / N_BIG:.3f} %)")
        check(got, expected_from_m(feats, m, rows, 100), f"1 M rows [{mode}]")
        answers.append(got)
        assert after["queries"] - before["queries"] == 1
        if mode == "replica on":
            assert 0 < exact < N_BIG, exact
            got = _call(eng, rows=rows, exclude=[5, 6], where=WHERE, topn=100)          # the other shapes on many workgroups
            check(got, expected_from_m(feats, m, rows + [5, 6], 100, WHERE), "1 M rows, by row, composed")
        else:
            assert exact == N_BIG, exact
    check(answers[1], answers[0], "1 M rows: replica on against off")


def test_the_cut_runs_up_to_ten_members_and_not_beyond(engine_lib):
    """K = 10 is the top of the pre-filter's range (kL1CutMaxK, csrc/engine_playlist.hip.h): with the replica fewer rows than the
    catalogue has take the chains there; from K = 11 on the launch gets no replica and every row does.  Either way the answer is
    the oracle's and the replica-off handle's, bit for bit."""
    n = 70_001
    feats = oracle.mt19937_uniform(25, n)
    rng = np.random.default_rng(25)
    cases = []
    for k in (7, 10, 11):
        rows = [int(r) for r in rng.choice(n, size=k, replace=False)]
        cases.append((k, rows, mean_l1(feats, feats[rows])))
    answers = {}
    for mode, eng in _engines(feats):
        for k, rows, m in cases:
            before = eng.playlist_counters()["rows_exact"]
            got = _call(eng, rows=rows, topn=100)
            exact = eng.playlist_counters()["rows_exact"] - before
            print(f"[{mode}] K = {k}: rows_exact {exact} of {n}")
            check(got, expected_from_m(feats, m, rows, 100), f"K = {k} [{mode}]")
            answers.setdefault(k, []).append(got)
            if mode == "replica on" and k <= 10:
                assert 0 < exact < n, (k, exact)
            else:
                assert exact == n, (mode, k, exact)
    for k, (off, on) in answers.items():
        check(on, off, f"K = {k}: replica on against off")


def test_lanes_updates_rebuild_and_interleaving(engine_lib):
    """A lane gives its parent's bits; playlist, distance and any-of requests before and after a Manhattan request on the same
    handle (one staging buffer, one shared threshold word, one norms array) return the bits they returned before it; after
    update_rows on a few rows, and after rebuild_replica (which drops the norms), the call equals a fresh handle's."""
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    n = 70_001
    feats = oracle.mt19937_uniform(24, n)
    rows = [7, 7_000, 69_999]
    m = mean_l1(feats, feats[rows])
    want = expected_from_m(feats, m, rows + [8, 9], 200, WHERE)
    with CosineEngine(feats) as eng:
        eng.set_replica(capi.REPLICA_ON)
        cos_before = eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE)
        dist_before = eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE)
        any_before = engine.query_anyof(eng, 200, rows=rows, exclude=[8, 9], where=WHERE)
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent")
        check(engine.query_manhattan(eng, 200, rows=rows, exclude=[8, 9], where=WHERE), want, "the Python function")
        check_scores(eng.query_playlist_topn(rows, 300, [8, 9], where=WHERE), cos_before, "cosine by row after a Manhattan request")
        check_scores(eng.query_nearest_rows(rows, 200, [8, 9], where=WHERE), dist_before, "distance after a Manhattan request")
        any_after = engine.query_anyof(eng, 200, rows=rows, exclude=[8, 9], where=WHERE)
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(any_after, any_before)), "any-of after a Manhattan request"
        lane = eng.lane()
        try:
            check(_call(lane, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "lane")
            check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want, "parent, after the lane's call")
        finally:
            lane.close()
        # a few rows change in place (some of them onto a member): the call answers as a fresh handle does
        rng = np.random.default_rng(71)
        changed_rows = np.sort(rng.choice(n, size=50, replace=False))
        changed = feats.copy()
        changed[changed_rows] = rng.random((changed_rows.size, 12), dtype=np.float32)
        changed[changed_rows[:20]] = feats[7] * np.float32(1.01)
        eng.update_rows(changed_rows, changed[changed_rows])
        m2 = mean_l1(changed, changed[rows])
        want2 = expected_from_m(changed, m2, rows + [8, 9], 200, WHERE)
        check(_call(eng, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "after update_rows")
    with CosineEngine(changed) as fresh:   # (a handle that never had a lane: one that had cannot rebuild its replicas)
        fresh.set_replica(capi.REPLICA_ON)
        check(_call(fresh, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "a fresh handle")
        before = fresh.playlist_counters()["rows_exact"]
        fresh.rebuild_replica()                                       # drops the norms: the next request builds them again
        check(_call(fresh, rows=rows, exclude=[8, 9], where=WHERE, topn=200), want2, "after rebuild_replica")
        assert fresh.playlist_counters()["rows_exact"] - before < n, "the pre-filter is on again after the rebuild"


@pytest.mark.parametrize("placement", ["sharded", "replicated"])
def test_node_handles_on_one_gpu(engine_lib, placement):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 140_001
    feats = oracle.mt19937_uniform(11, n)
    feats[n - 5:] = feats[17]                                     # ties across the two shards
    lab = uniform_labels(n, 30, 9)
    rng = np.random.default_rng(10)
    seen = sorted({int(r) for r in rng.choice(n, size=n // 4, replace=False)})
    pl = capi.PLACEMENT_SHARDED if placement == "sharded" else capi.PLACEMENT_REPLICATED
    with NodeEngine(feats, devices=[0, 0], placement=pl) as node, CosineEngine(feats) as eng:
        fn = node._lib.mi355rec_sharded_query_manhattan_request
        node.set_labels(lab)
        eng.set_labels(lab)
        for k in (1, 6, 32):
            rows = [17] + [int(r) for r in rng.choice(n, size=k - 1, replace=False)]
            excl = rng.integers(0, n, size=300).tolist()
            m = mean_l1(feats, feats[rows])
            for topn in (10, 1024):
                for kw, excluded in ((dict(rows=rows, exclude=excl, where=WHERE, labels=[0, 7, 29]), rows + excl),
                                     (dict(members=feats[rows], exclude=excl), excl), (dict(rows=rows), rows)):
                    rc, ids, dist = request_call(capi, fn, node._h, topn=topn, **kw)
                    assert rc == capi.OK, node._lib.mi355rec_sharded_last_error(node._h)
                    what = f"{placement} K={k} top-{topn} {sorted(kw)}"
                    check((ids, dist), _call(eng, topn=topn, **kw), what + " against the single handle")
                    check((ids, dist), expected_from_m(feats, m, excluded, topn, kw.get("where"), lab, kw.get("labels")), what)
        m = mean_l1(feats, feats[[3, 4]])
        for kw, rs in ((dict(seen=seen), dict(rowset=seen, rowset_only=False)), (dict(only=seen), dict(rowset=seen, rowset_only=True))):
            got = engine.query_manhattan(node, 20, rows=[3, 4], **kw)
            check(got, engine.query_manhattan(eng, 20, rows=[3, 4], **kw), "the Python function, node against single handle")
            check(got, expected_from_m(feats, m, [3, 4], 20, **rs), "the Python function with a row set")
        rc = request_call(capi, fn, node._h, members=feats[:2], flags=1)[0]
        assert rc == capi.ERR_INVALID_ARG and "must be 0" in node._lib.mi355rec_sharded_last_error(node._h).decode()


def test_one_shard_forwards(engine_lib):
    import torch  # noqa: F401
    from spotify_recommender_amd import capi, engine
    from spotify_recommender_amd.engine import NodeEngine
    n = 9_001
    feats = hostile_catalogue(n)
    rows = [0, 100, 9_000]
    m = mean_l1(feats, feats[rows])
    with NodeEngine(feats, devices=[0], placement=capi.PLACEMENT_AUTO) as node:
        check(engine.query_manhattan(node, 50, rows=rows, exclude=[1], where=WHERE), expected_from_m(feats, m, rows + [1], 50, WHERE), "one shard")


def test_the_cli_answers_as_the_cpu_backend_does(engine_lib, tmp_path):
    """One `--distance manhattan` run on the GPU against the same run with no device visible (the CPU backend): the same
    recommendations and the same printed distances."""
    from spotify_recommender_amd import build
    from tests.test_playlist_cpu import _write_csv
    build.build_shim()
    _write_csv(tmp_path / "songs.csv")
    pre = subprocess.run([str(build.BIN_CLI), "--preprocess", "songs.csv"], capture_output=True, text=True, cwd=tmp_path)
    assert pre.returncode == 0, pre.stdout + pre.stderr
    ids = [l.split(",")[0] for l in (tmp_path / "songs.csv").read_text().splitlines()[1:]]
    args = [str(build.BIN_CLI), "--playlist", ",".join(ids[i] for i in (5, 70, 333)), "--distance", "manhattan", "-n", "12", "--where", "energy=0.1:0.9"]
    gpu = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
    cpu = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert gpu.returncode == 0 and cpu.returncode == 0, (gpu.stderr, cpu.stderr)
    tail = [p.stdout.split("Recommendations:", 1)[1] for p in (gpu, cpu)]
    assert tail[0] == tail[1] and len(re.findall(r"\(distance ", tail[0])) == 12, tail
    assert "=== NEAREST MODE (Manhattan distance) ===" in gpu.stdout
