"""What ROW UPDATES (include/mi355rec_diag.h) are checked with, shared by tests/test_gpu_update_rows.py and
tests/test_update_rows_cpu.py: the update lists and the hostile contents, and `check_routes`, which asks an engine
every route it has and compares each answer with the existing oracles run on the UPDATED numpy matrix (oracle.oracle,
tests/parity.py, playlist_oracle, distance_oracle, labels_oracle, prior_oracle).  Nothing of the engine makes an expectation."""
import numpy as np

from oracle import oracle
from tests import distance_oracle, labels_oracle, playlist_oracle, prior_oracle
from tests.parity import assert_canonical_order, assert_topn_matches

WANTED = [0, 2, 5]       # the label set of the label routes (labels are uniform in [0, 6))
PRIOR_WEIGHT = 0.25
SPECIAL_ROWS = {"zero": 0.0, "nan": np.nan, "huge": 1e20, "tiny": 1e-6}


def catalogue(n: int) -> np.ndarray:
    return oracle.mt19937_uniform(900 + n % 97, n)


def update_lists(n: int, rng):
    """The lists per size: row 0, row n - 1, a row of the last quad that is not the last row, a random tenth, all rows."""
    lists = {"first": [0], "last": [n - 1]}
    quad0 = (n - 1) // 4 * 4
    if quad0 < n - 1:
        lists["in the last quad"] = [quad0]
    tenth = max(1, n // 10)
    lists["a tenth"] = sorted(int(r) for r in rng.choice(n, size=tenth, replace=False))
    lists["all"] = [int(r) for r in rng.permutation(n)]
    return lists


def new_rows(cur, rows, q, rng):
    """The new features of an update list: random rows — but a list of ONE row (other than the query row q) becomes a copy of row
    q, so that the one changed row has to show at the head of every answer for q (a random row would almost never enter a top-10,
    and an engine that ignored the update would pass)."""
    new = rng.random((len(rows), 12), dtype=np.float32)
    if len(rows) == 1 and rows[0] != q:
        new[0] = cur[q]
    return new


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)


def check_single(got, cur, qvec, exclude, topn, what):
    """One query's (ids, scores) against the oracle: tests/parity.py's check, then ids and score bits equal."""
    idx, sc = got
    s = oracle.scores(cur, np.ascontiguousarray(qvec, np.float32))
    want_i, want_s = oracle.topn_canonical(s, int(exclude), topn)
    assert_topn_matches(idx, sc, s, int(exclude), topn, ref_idx=want_i)
    assert_canonical_order(idx, s)
    assert np.asarray(idx).tolist() == want_i.tolist(), f"{what}: ids differ"
    assert np.array_equal(_bits(sc), _bits(want_s)), f"{what}: score bits differ"


def check_routes(eng, cur, q, what, labels=None, priors=None, streamed=None, batches=(2, 12, 33)):
    """Every route of `eng` (a CosineEngine or a NodeEngine) against the oracles on `cur`, the matrix as it is now.
    streamed: None, or a callable (rows, topn) -> list of (ids, scores) that runs a stream of queries by row with a flush."""
    n = cur.shape[0]
    for topn in (1, 10):
        check_single(eng.query_row_topn(q, topn), cur, cur[q], q, topn, f"{what}: row query top-{topn}")
        check_single(eng.query_topn(cur[q], q, topn), cur, cur[q], q, topn, f"{what}: value query top-{topn}")
    qrows = [(q + 7 * i) % n for i in range(5)]
    if streamed is not None:
        for r, got in zip(qrows, streamed(qrows, 10)):
            check_single(got, cur, cur[r], r, 10, f"{what}: streamed query of row {r}")
    for b in batches:
        rows = np.asarray([(q + 3 * i) % n for i in range(b)], np.int64)
        idx, sc, counts = eng.query_batch_topn(cur[rows], rows, 10)
        for i, r in enumerate(rows):
            check_single((idx[i, :counts[i]], sc[i, :counts[i]]), cur, cur[r], int(r), 10, f"{what}: batch of {b}, query {i}")
    for k in (1, 3):
        members = sorted({(q + i) % n for i in range(k)})
        playlist_oracle_check = playlist_oracle.expected_rows(cur, members, None, 10)
        labels_oracle.check(eng.query_playlist_topn(members, 10), playlist_oracle_check, f"{what}: playlist K={k}")
        distance_oracle.check(eng.query_nearest_rows(members, 10), distance_oracle.expected_rows(cur, members, None, 10),
                              f"{what}: distance K={k}")
        if labels is not None:
            scores = prior_oracle.scores_of(cur, cur[members])
            labels_oracle.check(eng.query_playlist_topn(members, 10, labels=WANTED),
                                prior_oracle.expected_prior(scores, None, None, cur, labels, WANTED, members, 10),
                                f"{what}: playlist K={k} within labels")
        if priors is not None:
            scores = prior_oracle.scores_of(cur, cur[members])
            labels_oracle.check(eng.query_playlist_topn(members, 10, prior_weight=PRIOR_WEIGHT),
                                prior_oracle.expected_prior(scores, priors, PRIOR_WEIGHT, cur, None, None, members, 10),
                                f"{what}: playlist K={k} with priors")
    if labels is not None:
        labels_oracle.check(eng.query_row_topn_labels(q, WANTED, 10), labels_oracle.expected(cur, labels, cur[q], q, WANTED, 10),
                            f"{what}: label route")


def adversarial_steps(cur, q, topn, rng):
    """The deterministic hostile contents for the query row q, as (name, rows, new features) computed from the CURRENT
    matrix one step at a time (a generator: each step sees the steps before it applied to `cur` by the caller)."""
    n = cur.shape[0]
    s = oracle.scores(cur, cur[q])
    top_i, _ = oracle.topn_canonical(s, q, n)
    if top_i.size > topn:       # a row outside the top-N becomes a copy of row q: it must come first (a stale replica entry rules it out)
        r = int(top_i[-1])
        yield "a far row becomes the query", [r], cur[q][None, :].copy()
    if top_i.size > 1:          # the former best row becomes -q: it must vanish (a stale fp32 row keeps it)
        s = oracle.scores(cur, cur[q])
        best = int(oracle.topn_canonical(s, q, 1)[0][0])
        yield "the best row becomes -query", [best], -cur[q][None, :].copy()
    yield "the query row itself changes", [q], rng.random((1, 12), dtype=np.float32)
    if n >= 4:                  # (a row that is no member of check_routes' playlists: those are rows q, q + 1, q + 2)
        r = (q + (5 if n > 40 else 3)) % n
        for name, v in SPECIAL_ROWS.items():
            yield f"row {r} becomes all {name}", [r], np.full((1, 12), v, np.float32)
        yield f"row {r} becomes normal again", [r], rng.random((1, 12), dtype=np.float32)
