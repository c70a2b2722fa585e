"""DISTANCE REQUESTS on a host without a GPU (include/mi355rec_diag.h): mi355rec_sharded_query_distance_request served by the
product's CPU backend (csrc/cpu_backend.cpp) against tests/distance_oracle.py — equal ids, bit-equal distances, equal counts,
the padding — plus every refusal with its message, the short structs and the bindings."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from tests.distance_oracle import (check, cross_check, expected_from_m, hostile_catalogue, mean_sqdist, request_call)
from tests.playlist_labels_oracle import uniform_labels


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")

SIZES = (1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [1, 4, 4, 9]


def _fn(nd):
    return nd._lib.mi355rec_sharded_query_distance_request


def _call(nd, **kw):
    from spotify_recommender_amd import capi
    rc, ids, dist = request_call(capi, _fn(nd), nd._h, **kw)
    assert rc == capi.OK, nd._lib.mi355rec_sharded_last_error(nd._h)
    return ids, dist


@pytest.mark.parametrize("n", SIZES)
def test_parity(engine_lib, n):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(n)
    lab = uniform_labels(n, 12, 3, unlabelled=0.05)
    rng = np.random.default_rng([7, n])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(lab)
        for k in (1, 3, 32):
            rows = [int(r) for r in rng.choice(n, size=min(k, n), replace=False)]
            if 0 not in rows:
                rows[0] = 0                                          # row 0 has duplicates: distance 0, ties by row
            vecs = rng.random((k, 12), dtype=np.float32)
            vecs[0] = feats[0]
            hostile_vecs = vecs.copy()
            hostile_vecs[k // 2, 3] = np.float32(1e-30)
            for what, kw, members, excluded in (("by value", dict(members=vecs), vecs, []),
                                                ("by row", dict(rows=rows), feats[rows], rows),
                                                ("tiny member", dict(members=hostile_vecs), hostile_vecs, [])):
                m = mean_sqdist(feats, members)
                cross_check(feats, members, m)
                n_adm = int(expected_from_m(feats, m, excluded, n)[0].size)
                excl = [0, 0, n // 2, n - 1]
                n_adm_x = int(expected_from_m(feats, m, excluded + excl, n)[0].size)
                for topn in sorted({1, 10, 1024, max(1, min(1024, n_adm)), min(1024, n_adm + 1)}):
                    tag = f"n={n} k={k} {what} top-{topn}"
                    got = _call(nd, topn=topn, **kw)
                    check(got, expected_from_m(feats, m, excluded, topn), tag)
                    assert got[0].size == min(topn, n_adm)
                    check(_call(nd, topn=topn, exclude=excl, **kw), expected_from_m(feats, m, excluded + excl, topn), tag + " exclude")
                    check(_call(nd, topn=topn, where=WHERE, **kw), expected_from_m(feats, m, excluded, topn, WHERE), tag + " filter")
                    check(_call(nd, topn=topn, labels=WANTED, **kw), expected_from_m(feats, m, excluded, topn, None, lab, WANTED), tag + " labels")
                    check(_call(nd, topn=topn, exclude=excl, where=WHERE, labels=WANTED, **kw),
                          expected_from_m(feats, m, excluded + excl, topn, WHERE, lab, WANTED), tag + " all together")
                for topn in {max(1, min(1024, n_adm_x)), min(1024, n_adm_x + 1)}:
                    check(_call(nd, topn=topn, exclude=excl, **kw), expected_from_m(feats, m, excluded + excl, topn), f"n={n} k={k} {what} eff")
            # members that are not finite: no row has a finite m, nothing is listed
            bad = vecs.copy()
            bad[0, 0] = np.nan
            ids, dist = _call(nd, members=bad, topn=10)
            assert ids.size == 0
            bad[0, 0] = np.inf
            assert _call(nd, members=bad, topn=10)[0].size == 0


def test_duplicates_tie_by_row_and_report_zero(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(257)
    dups = [i for i in range(257) if np.array_equal(feats[i], feats[0])]
    assert len(dups) >= 5
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        ids, dist = _call(nd, members=feats[:1], topn=len(dups))
        assert ids.tolist() == dups and not dist.view(np.uint32).any()      # +0.0f, never -0.0f
        ids, dist = _call(nd, rows=[0], topn=len(dups))
        assert ids.tolist() == dups[1:] + [int(ids[-1])] and not dist[:-1].view(np.uint32).any() and dist[-1] > 0


def test_refusals(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(300)
    v = feats[:2]
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        def refused(msg, **kw):
            rc = request_call(capi, _fn(nd), nd._h, **kw)[0]
            text = nd._lib.mi355rec_sharded_last_error(nd._h).decode()
            assert rc == capi.ERR_INVALID_ARG and msg in text, (sorted(kw), rc, text)

        for flags in (1, 2, 4, 8, 0x80000000):
            refused("in a distance query: must be 0", members=v, flags=flags)
        refused("members by value and by row in one distance query", members=v, rows=[1, 2])
        refused("a distance query needs members by value or by row", topn=10)
        full = ctypes.sizeof(capi.DistanceQuery)
        assert full == 64
        for size in (0, 2, 6, 12, 47, 50, 63, full + 1, full + 8, 88):
            refused(f"distance query of size {size}: not the end of a field", members=v, size=size)
        refused("has no labels", members=v, labels=[1])
        nd.set_labels(np.zeros(300, np.int32))
        refused("n_labels must be positive", members=v, labels=[])
        refused("n_labels must be positive", members=v, labels=[1], n_labels=-1)
        refused("null label set", members=v, n_labels=2)
        refused("label 1024 out of", members=v, labels=[3, 1024])
        refused("label -1 out of", members=v, labels=[-1])
        for k in (0, -1, 33):
            refused(f"playlist of {k} songs", members=np.zeros((40, 12), np.float32), k=k)
        for topn in (0, -3, 1025):
            refused(f"topn {topn} out of [1, 1024]", members=v, topn=topn)
        refused("n_exclude -1 out of", members=v, n_exclude=-1)
        refused("n_exclude 1025 out of", members=v, exclude=list(range(300)) * 4, n_exclude=1025)
        refused("null exclusion list with n_exclude 3", members=v, n_exclude=3)
        refused("excluded row 300 out of the catalogue", members=v, exclude=[300])
        refused("excluded row -1 out of the catalogue", members=v, exclude=[-1])
        refused("Invalid song index: 300", rows=[1, 300])
        refused("Invalid song index: -1", rows=[-1])
        bad = capi.Filter()
        bad.active = 1 << 12
        q = capi.DistanceQuery(size=full, members=v.ctypes.data_as(ctypes.c_void_p), k=2, topn=5, filter=ctypes.pointer(bad))
        idx = np.zeros(5, np.int64)
        res = capi.DistanceResult(idx.ctypes.data_as(ctypes.c_void_p), None, None)
        assert _fn(nd)(nd._h, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG
        # null structs, a null out_idx; out_distance and out_count may be null
        assert _fn(nd)(nd._h, None, ctypes.byref(res)) == capi.ERR_INVALID_ARG
        assert _fn(nd)(nd._h, ctypes.byref(q), None) == capi.ERR_INVALID_ARG
        q.filter = None
        assert _fn(nd)(nd._h, ctypes.byref(q), ctypes.byref(capi.DistanceResult(None, None, None))) == capi.ERR_INVALID_ARG
        assert _fn(nd)(nd._h, ctypes.byref(q), ctypes.byref(res)) == capi.OK
        assert idx.tolist() == _call(nd, members=v, topn=5)[0].tolist()
        assert _fn(nd)(None, ctypes.byref(q), ctypes.byref(res)) == capi.ERR_INVALID_ARG


def test_short_structs_read_later_fields_as_zero(engine_lib):
    """A struct cut where a field ends behaves as the full struct with the later fields zero."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(300)
    lab = uniform_labels(300, 12, 3)
    v = feats[5:8]
    kw = dict(members=v, exclude=[1, 2, 3], where=WHERE, labels=WANTED, topn=10)
    ends = [(f[0], getattr(capi.DistanceQuery, f[0]).offset) for f in capi.DistanceQuery._fields_][1:] + [("(end)", 64)]
    assert [e for _, e in ends] == [4, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64]
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        nd.set_labels(lab)
        for name, size in ends:
            rc, ids, dist = request_call(capi, _fn(nd), nd._h, size=size, **kw)
            text = nd._lib.mi355rec_sharded_last_error(nd._h).decode()
            if size <= 8:            # flags and members zero: neither members nor rows
                assert rc == capi.ERR_INVALID_ARG and "needs members" in text, (name, text)
            elif size <= 48:         # ... up to labels: k is zero
                assert rc == capi.ERR_INVALID_ARG and "playlist of 0 songs" in text, (name, text)
            elif size <= 60:         # k (and n_exclude, n_labels) read, topn zero
                assert rc == capi.ERR_INVALID_ARG and ("topn 0 out of" in text or "n_labels must be positive" in text
                                                       or "null exclusion list" in text), (name, text)
            else:
                assert rc == capi.OK
                check((ids, dist), _call(nd, **kw), "the full struct")
        # a caller that knows the struct only up to n_exclude cannot exist (topn lies behind it); one that passes zeros for
        # the optional pointers is the plain call
        check(_call(nd, members=v, topn=10), _call(nd, members=v, topn=10, exclude=[], n_exclude=0), "zeros")


def test_bindings(engine_lib):
    """include/mi355rec_diag.h, capi.SIGNATURES, the ctypes structs and the engine classes agree."""
    from pathlib import Path

    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import CosineEngine, NodeEngine
    header = (Path(capi.__file__).resolve().parents[1] / "include" / "mi355rec_diag.h").read_text()
    assert "DISTANCE REQUESTS" in header
    body = re.search(r"typedef struct \{([^}]*)\} mi355rec_distance_query_t;", header).group(1)
    names = [n for line in body.splitlines() for n in re.findall(r"[\s*](\w+)\s*(?:,|;)", line.split("/*")[0])]
    assert names == [f[0] for f in capi.DistanceQuery._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} mi355rec_distance_result_t;", header).group(1)
    names = [n for line in body.splitlines() for n in re.findall(r"[\s*](\w+)\s*(?:,|;)", line.split("/*")[0])]
    assert names == [f[0] for f in capi.DistanceResult._fields_]
    assert ctypes.sizeof(capi.DistanceQuery) == 64 and ctypes.sizeof(capi.DistanceResult) == 24
    for name in ("mi355rec_query_distance_request", "mi355rec_sharded_query_distance_request"):
        assert re.search(r"\bint " + name + r"\(", header)
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == 3
        assert hasattr(engine_lib, name)
    for cls in (CosineEngine, NodeEngine):
        for name in ("query_nearest", "query_nearest_rows"):
            assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == ["members" if name == "query_nearest" else "rows", "topn",
                                                                                   "exclude", "where", "labels"]


def test_python_methods(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = hostile_catalogue(2049)
    lab = uniform_labels(2049, 12, 3)
    rows = [5, 777, 2000]
    m = mean_sqdist(feats, feats[rows])
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd:
        nd.set_labels(lab)
        check(nd.query_nearest(feats[rows], 20), expected_from_m(feats, m, [], 20), "by value")
        check(nd.query_nearest_rows(rows, 20), expected_from_m(feats, m, rows, 20), "by row")
        check(nd.query_nearest_rows(rows, 20, exclude=[1, 2], where=WHERE, labels=set(WANTED)),
              expected_from_m(feats, m, rows + [1, 2], 20, WHERE, lab, WANTED), "everything")
        # k = 1: the Euclidean distance itself
        ids, dist = nd.query_nearest(feats[20], 5)
        want = np.sqrt(((feats[ids].astype(np.float64) - feats[20].astype(np.float64)) ** 2).sum(axis=1))
        assert ids[0] == 20 and np.allclose(dist, want, rtol=1e-6, atol=0)
        with pytest.raises(capi.Mi355Error, match="topn 0 out of"):
            nd.query_nearest(feats[20], 0)


# ---- the drop-in CLI ------------------------------------------------------------------------------------------------
def _run(args, cwd):
    import subprocess

    from spotify_recommender_amd import build
    return subprocess.run([str(build.BIN_CLI), *args], capture_output=True, text=True, cwd=cwd)


def _recommended(stdout):
    out = stdout.split("Recommendations:", 1)[1]
    ids = [l.split("ID:", 1)[1].strip() for l in out.splitlines() if l.strip().startswith("ID:")]
    dist = [float(m) for m in re.findall(r"\(distance ([-+0-9.einfa]+)\)", out)]
    return ids, dist


def test_cli_metric_euclidean(engine_lib, golden_dir, tmp_path):
    import shutil

    from spotify_recommender_amd import build
    build.build_shim()
    shutil.copy(golden_dir / "sample_songs.csv", tmp_path / "songs.csv")
    p = _run(["--preprocess", "songs.csv"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    seed = "5SuOikwiRyPMVoIQDJUgSV"
    p = _run(["--id", seed, "-n", "1000", "--metric", "euclidean"], tmp_path)
    assert p.returncode == 0 and "NEAREST MODE" in p.stdout, p.stdout + p.stderr
    ids, dist = _recommended(p.stdout)
    assert len(ids) == 3 and seed not in ids and len(dist) == 3 and dist == sorted(dist) and dist[0] >= 0
    # the same song as a one-song playlist, and cosine named explicitly is the default mode
    q = _run(["--playlist", seed, "-n", "1000", "--metric", "euclidean"], tmp_path)
    assert q.returncode == 0 and _recommended(q.stdout) == (ids, dist), q.stdout + q.stderr
    c = _run(["--id", seed, "-n", "3", "--metric", "cosine"], tmp_path)
    assert c.returncode == 0 and "NEAREST MODE" not in c.stdout and "(distance" not in c.stdout, c.stdout + c.stderr
    # with --genre and --where
    g = _run(["--playlist", seed, "-n", "3", "--metric", "euclidean", "--genre", "rock", "--genre", "dance", "--where", "energy=0:1"], tmp_path)
    assert g.returncode == 0 and "Restricted to genres: rock dance" in g.stdout, g.stdout + g.stderr
    got = _recommended(g.stdout)[0]
    assert got and set(got) <= set(ids)
    # refusals exit 1 with a message
    for extra, msg in ((["--diverse", "0.5"], "--diverse"), (["--weights", "1"], "--weights"), (["--dislike", "dupA"], "--dislike"),
                       (["--priors", "p.txt", "--prior-weight", "1"], "--priors"), (["--max-per-artist", "1"], "--max-per-artist")):
        r = _run(["--playlist", seed, "--metric", "euclidean", *extra], tmp_path)
        assert r.returncode == 1 and "--metric euclidean cannot be combined with " + msg in r.stderr, (extra, r.stderr)
    r = _run(["--id", seed, "--metric", "manhattan"], tmp_path)
    assert r.returncode == 1 and "cosine or euclidean" in r.stderr
    r = _run(["--id", seed, "--metric"], tmp_path)
    assert r.returncode == 1 and "--metric needs a name" in r.stderr
    assert "--metric euclidean" in _run([], tmp_path).stdout
