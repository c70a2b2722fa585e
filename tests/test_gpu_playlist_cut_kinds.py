"""Every kind of the playlist pre-filter's cut on the MI355X (csrc/playlist_cut.hip.h: plain, prior, distance, scaled, and off),
one request per kind: the answer bit for bit against the kind's oracle, and the pre-filter's DECISIONS against the commit that
came before the cut was moved into pieces.  The only observable of those decisions besides speed is the rows_exact counter
(mi355rec_playlist_counters), and it depends on the order in which workgroups publish thresholds, so the shapes here launch ONE
workgroup (with a replica the grid is ceil(tiles / 8)): the counter is then a function of the request alone.

    n = 4 093    two tiles, a last quad of one row, fewer rows than the anchor table holds
    n = 12 289   seven tiles, a last quad of one row

Rows: tests/golden/catalogue4096.npz (a NaN row, a zero row, tiny rows: the replica's special rows), tiled with a seeded relative
perturbation for the larger n.  Replica on, top-10 and top-100, K = 1, 3, 32 members by row.

PARENT_ROWS_EXACT holds what the parent commit's library (5c8349c) counted for each request, measured on an MI355X by running this
file as a script with MI355REC_LIB naming that library, twice, with equal counts in both runs for every case (docs/LAB_NOTES.md).
A scaled distance request has no cut (it runs on the exact path): its count is n, nothing ruled out."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tests import distance_oracle, scaled_oracle  # noqa: E402
from tests.playlist_labels_oracle import expected_scored, scores_of, uniform_labels  # noqa: E402
from tests.prior_oracle import blended  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (4_093, 12_289)
TOPNS = (10, 100)
KS = (1, 3, 32)
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
WANTED = [0, 2, 5]
N_LABELS = 6
DROP_ONE = np.ones(12, np.float32)
DROP_ONE[2] = 0                                     # one feature dropped
# name: (metric, request arguments); "signed": weights of both signs, made per K
REQUESTS = {
    "plain": ("cosine", {}),
    "plain signed": ("cosine", {"weights": "signed"}),
    "prior +4": ("cosine", {"prior_weight": 4.0}),
    "prior -4": ("cosine", {"prior_weight": -4.0}),
    "prior 0.25": ("cosine", {"prior_weight": 0.25}),
    "distance": ("euclidean", {}),
    "scaled general": ("cosine", {"scales": scaled_oracle.GENERAL}),
    "scaled one dropped": ("cosine", {"scales": DROP_ONE}),
    "scaled distance": ("euclidean", {"scales": scaled_oracle.GENERAL}),
    "plain filtered": ("cosine", {"where": WHERE}),
    "plain labelled": ("cosine", {"labels": WANTED}),
}


@functools.lru_cache(maxsize=None)
def catalogue(n):
    """(rows, labels, priors) of the shape n: the same in the test and in the script that measured the parent."""
    base = np.ascontiguousarray(np.load(Path(__file__).resolve().parent / "golden" / "catalogue4096.npz")["feats"], np.float32)
    rng = np.random.default_rng(n)
    reps = -(-n // base.shape[0])
    feats = np.tile(base, (reps, 1))
    with np.errstate(invalid="ignore"):
        feats[base.shape[0]:] *= (1 + 0.05 * rng.standard_normal((feats.shape[0] - base.shape[0], 12))).astype(np.float32)
    feats = np.ascontiguousarray(feats[:n], np.float32)
    return feats, uniform_labels(n, N_LABELS, n, unlabelled=0.1), (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def members_of(n, k):
    """K distinct rows with an ordinary norm (a hostile member switches the pre-filter off: not what this file is about)."""
    feats = catalogue(n)[0]
    norm = np.sqrt((feats.astype(np.float64) ** 2).sum(axis=1))
    good = np.flatnonzero(np.isfinite(norm) & (norm > 0.5))
    return tuple(int(r) for r in np.random.default_rng(1000 * k + n).choice(good, size=k, replace=False))


def weights_of(k):
    w = np.random.default_rng(k).uniform(0.25, 2.0, size=k).astype(np.float32)
    w[1::3] *= np.float32(-0.5)                     # (K = 1: a single like)
    return w


@functools.lru_cache(maxsize=None)
def reference(n, k, what):
    """The oracle's ranking values of every row, once per member set: shared by the requests and both top-N."""
    feats = catalogue(n)[0]
    members = feats[list(members_of(n, k))]
    if what == "cosine":
        return scores_of(feats, members)
    if what == "cosine signed":
        return scores_of(feats, members, weights_of(k))
    if what == "distance":
        return distance_oracle.mean_sqdist(feats, members)
    if what == "scaled distance":
        return scaled_oracle.distance_m(feats, members, scaled_oracle.GENERAL)
    return scaled_oracle.cosine_scores(feats, members, REQUESTS[what][1]["scales"])


def expected(n, k, name, topn):
    feats, labels, priors = catalogue(n)
    metric, args = REQUESTS[name]
    rows = list(members_of(n, k))
    if metric == "euclidean":
        m = reference(n, k, "scaled distance" if "scales" in args else "distance")
        return distance_oracle.expected_from_m(feats, m, rows, topn)
    if "scales" in args:
        return scaled_oracle.cosine_expected(reference(n, k, name), feats, rows, topn)
    scores = reference(n, k, "cosine signed" if "weights" in args else "cosine")
    if "prior_weight" in args:
        scores = blended(scores, priors, args["prior_weight"])
    return expected_scored(scores, feats, labels, args.get("labels"), rows, topn, args.get("where"))


def ask(eng, n, k, name, topn):
    """((ids, values), the rows_exact the request added)."""
    metric, args = REQUESTS[name]
    args = dict(args)
    if "weights" in args:
        args["weights"] = weights_of(k)
    rows = np.asarray(members_of(n, k), np.int64)
    before = eng.playlist_counters()["rows_exact"]
    if metric == "euclidean":
        got = eng.query_nearest_rows_scaled(rows, topn, args["scales"]) if "scales" in args else eng.query_nearest_rows(rows, topn)
    else:
        got = eng.query_playlist_topn(rows, topn, **args)
    return got, eng.playlist_counters()["rows_exact"] - before


def engine(n):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    feats, labels, priors = catalogue(n)
    eng = CosineEngine(feats)
    eng.set_replica(capi.REPLICA_ON)
    eng.set_labels(labels)
    eng.set_priors(priors)
    return eng


# the parent commit's counts (see the docstring): (n, K, request) -> rows_exact added at (top-10, top-100)
PARENT_ROWS_EXACT = {
    (4093, 1, 'plain'): (298, 422),
    (4093, 1, 'plain signed'): (298, 422),
    (4093, 1, 'prior +4'): (390, 1176),
    (4093, 1, 'prior -4'): (332, 1077),
    (4093, 1, 'prior 0.25'): (276, 745),
    (4093, 1, 'distance'): (284, 427),
    (4093, 1, 'scaled general'): (496, 755),
    (4093, 1, 'scaled one dropped'): (328, 518),
    (4093, 1, 'scaled distance'): (4093, 4093),
    (4093, 1, 'plain filtered'): (306, 645),
    (4093, 1, 'plain labelled'): (281, 417),
    (4093, 3, 'plain'): (312, 485),
    (4093, 3, 'plain signed'): (295, 445),
    (4093, 3, 'prior +4'): (403, 1221),
    (4093, 3, 'prior -4'): (454, 1132),
    (4093, 3, 'prior 0.25'): (290, 997),
    (4093, 3, 'distance'): (289, 478),
    (4093, 3, 'scaled general'): (510, 750),
    (4093, 3, 'scaled one dropped'): (408, 669),
    (4093, 3, 'scaled distance'): (4093, 4093),
    (4093, 3, 'plain filtered'): (317, 547),
    (4093, 3, 'plain labelled'): (287, 457),
    (4093, 32, 'plain'): (306, 525),
    (4093, 32, 'plain signed'): (317, 509),
    (4093, 32, 'prior +4'): (393, 1233),
    (4093, 32, 'prior -4'): (364, 1204),
    (4093, 32, 'prior 0.25'): (288, 1021),
    (4093, 32, 'distance'): (301, 505),
    (4093, 32, 'scaled general'): (574, 903),
    (4093, 32, 'scaled one dropped'): (400, 791),
    (4093, 32, 'scaled distance'): (4093, 4093),
    (4093, 32, 'plain filtered'): (390, 739),
    (4093, 32, 'plain labelled'): (311, 461),
    (12289, 1, 'plain'): (333, 722),
    (12289, 1, 'plain signed'): (333, 722),
    (12289, 1, 'prior +4'): (472, 1411),
    (12289, 1, 'prior -4'): (554, 1374),
    (12289, 1, 'prior 0.25'): (309, 932),
    (12289, 1, 'distance'): (351, 718),
    (12289, 1, 'scaled general'): (409, 900),
    (12289, 1, 'scaled one dropped'): (388, 930),
    (12289, 1, 'scaled distance'): (12289, 12289),
    (12289, 1, 'plain filtered'): (528, 1597),
    (12289, 1, 'plain labelled'): (334, 665),
    (12289, 3, 'plain'): (397, 930),
    (12289, 3, 'plain signed'): (333, 779),
    (12289, 3, 'prior +4'): (474, 1385),
    (12289, 3, 'prior -4'): (590, 1319),
    (12289, 3, 'prior 0.25'): (313, 1176),
    (12289, 3, 'distance'): (389, 942),
    (12289, 3, 'scaled general'): (1102, 2205),
    (12289, 3, 'scaled one dropped'): (727, 1471),
    (12289, 3, 'scaled distance'): (12289, 12289),
    (12289, 3, 'plain filtered'): (467, 1617),
    (12289, 3, 'plain labelled'): (351, 820),
    (12289, 32, 'plain'): (378, 1058),
    (12289, 32, 'plain signed'): (390, 995),
    (12289, 32, 'prior +4'): (600, 1374),
    (12289, 32, 'prior -4'): (577, 1432),
    (12289, 32, 'prior 0.25'): (316, 1225),
    (12289, 32, 'distance'): (364, 970),
    (12289, 32, 'scaled general'): (1223, 2231),
    (12289, 32, 'scaled one dropped'): (660, 1806),
    (12289, 32, 'scaled distance'): (12289, 12289),
    (12289, 32, 'plain filtered'): (403, 1633),
    (12289, 32, 'plain labelled'): (388, 839),
}


@pytest.mark.parametrize("n", SIZES)
def test_every_cut_kind_answers_as_its_oracle_and_decides_as_the_parent_commit(engine_lib, n):
    assert -(-(-(-(-(-n // 4)) // 512)) // 8) == 1 and n % 4 == 1   # one workgroup (ceil(tiles / 8)), a last quad of one row
    with engine(n) as eng:
        for k in KS:
            for name in REQUESTS:
                for topn, parent in zip(TOPNS, PARENT_ROWS_EXACT[(n, k, name)]):
                    got, exact = ask(eng, n, k, name, topn)
                    what = f"{n} rows, K = {k}, top-{topn}, {name}"
                    print(f"{what}: rows_exact {exact} (parent {parent})")
                    distance_oracle.check(got, expected(n, k, name, topn), what)
                    assert exact == parent, what
                    if name == "scaled distance":
                        assert exact == n, what     # the exact path: nothing ruled out


if __name__ == "__main__":   # the measurement: MI355REC_LIB=<the parent's library> python tests/test_gpu_playlist_cut_kinds.py
    for size in SIZES:
        with engine(size) as e:
            for members in KS:
                for request in REQUESTS:
                    print(f"    ({size}, {members}, {request!r}): ({', '.join(str(ask(e, size, members, request, t)[1]) for t in TOPNS)}),")
