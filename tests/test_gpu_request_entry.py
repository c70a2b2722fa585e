"""The request entry points on the MI355X after they became one body per handle type (csrc/engine_playlist.hip.h: request_entry;
csrc/sharded.hip: node_request_entry) over one struct conversion (csrc/playlist_request.h: from_request): a single handle, a node
handle over one device and a node handle over two virtual shards of it, each of the four kinds of request on each.

  * the conversion-level cases of tests/request_refusal_cases.py come back with the CPU fixture's exact text and code
    (tests/golden/request_refusals.json): the conversion is shared and neither handle type decorates its message;
  * one good request by row (k = 3, top-10, an exclusion list, a filter, a `seen=` row set) answers what the kind's CPU oracle gives,
    bit for bit;
  * the _candidates and score_*_candidates forms of the playlist and the distance request over a 20-id list with a duplicate and ids of
    both virtual shards answer their oracles.

300 rows: below the replica threshold, several quads, one tile; the node's shards hold 150 rows each."""
import pytest

from tests import anyof_oracle, candidate_scores_oracle, distance_oracle, manhattan_oracle, playlist_labels_oracle
from tests import request_refusal_cases as cases
from tests.candidates_oracle import gone

pytestmark = pytest.mark.gpu

N = cases.N_ROWS
ROWS = [5, 151, 298]
EXCLUDE = [7, 8, 200]
WHERE = {"energy": (0.1, 0.8), 2: (0.0, 0.7)}
SEEN = list(range(10, 120, 3)) + [160, 250]
LIST = [3, 149, 150, 299, 17, 42, 42, 77, 101, 120, 133, 160, 181, 200, 222, 240, 251, 263, 280, 8]   # 42 twice; both shards; 200 and 8 excluded


def _feats():
    feats = cases.catalogue()
    feats[N - 1] = feats[3]          # ties by row, across the two virtual shards
    feats[N // 2] = feats[3]
    return feats


@pytest.fixture(scope="module")
def handles(engine_lib):
    """[(name, engine, C prefix, {"mine", "foreign"} row set pointers)] over one catalogue."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.engine import NodeEngine
    feats = _feats()
    with CosineEngine(feats) as eng, NodeEngine(feats, devices=[0]) as one, NodeEngine(feats, devices=[0, 0]) as two:
        assert two.info()["shard_rows"] == [N // 2, N // 2]
        with eng.row_set([1, 2]) as s_eng, one.row_set([1, 2]) as s_one, two.row_set([1, 2]) as s_two:
            yield feats, [("single handle", eng, "mi355rec_", {"mine": s_eng._ptr(), "foreign": s_one._ptr()}),
                          ("node over [0]", one, "mi355rec_sharded_", {"mine": s_one._ptr(), "foreign": s_two._ptr()}),
                          ("node over [0, 0]", two, "mi355rec_sharded_", {"mine": s_two._ptr(), "foreign": s_one._ptr()})]


@pytest.mark.parametrize("kind", cases.KINDS)
def test_conversion_refusals_are_the_fixture(handles, kind):
    from spotify_recommender_amd import capi
    want = {name: cases.fixture()[kind][name] for name, _, conversion in cases.cases(capi, kind) if conversion}
    assert len(want) > 30
    for what, eng, prefix, sets in handles[1]:
        got = cases.run(capi, eng._lib, prefix, eng._h, kind, sets, conversion_only=True)
        assert list(got) == list(want)
        for name in want:
            assert got[name] == want[name], (what, kind, name)


def _pair(got, want, what):
    distance_oracle.check(got, want, what)   # equal ids, bit-equal values


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_good_request_is_the_oracle(handles, kind):
    from spotify_recommender_amd.engine import query_anyof, query_manhattan
    feats, engines = handles
    if kind == "playlist":
        want = playlist_labels_oracle.expected_rows(feats, None, ROWS, None, EXCLUDE + SEEN, 10, WHERE)
    elif kind == "distance":
        want = distance_oracle.expected_rows(feats, ROWS, EXCLUDE + SEEN, 10, WHERE)
    elif kind == "anyof":
        want = anyof_oracle.expected_rows(feats, ROWS, EXCLUDE, 10, where=WHERE, rowset=SEEN, rowset_only=False)
    else:
        want = manhattan_oracle.expected_rows(feats, ROWS, EXCLUDE, 10, where=WHERE, rowset=SEEN, rowset_only=False)
    assert len(want[0]) == 10
    for what, eng, _, _ in engines:
        if kind == "playlist":
            _pair(eng.query_playlist_topn(ROWS, 10, exclude=EXCLUDE, where=WHERE, seen=SEEN), want, what)
        elif kind == "distance":
            _pair(eng.query_nearest_rows_scaled(ROWS, 10, None, exclude=EXCLUDE, where=WHERE, seen=SEEN), want, what)
        elif kind == "anyof":
            anyof_oracle.check(query_anyof(eng, 10, rows=ROWS, exclude=EXCLUDE, where=WHERE, seen=SEEN), want, what)
        else:
            manhattan_oracle.check(query_manhattan(eng, 10, rows=ROWS, exclude=EXCLUDE, where=WHERE, seen=SEEN), want, what)


def test_the_list_forms_are_their_oracles(handles):
    from spotify_recommender_amd.engine import candidate_scores, with_candidates
    feats, engines = handles
    assert len(LIST) == 20 and len(set(LIST)) == 19 and min(LIST) < N // 2 <= max(LIST)
    out = gone(N, LIST, EXCLUDE).tolist()
    top_cosine = playlist_labels_oracle.expected_rows(feats, None, ROWS, None, out, 10)
    top_distance = distance_oracle.expected_rows(feats, ROWS, out, 10)
    all_cosine = candidate_scores_oracle.expected(N, LIST, playlist_labels_oracle.scores_of(feats, feats[ROWS]), EXCLUDE + ROWS)
    all_distance = candidate_scores_oracle.expected(N, LIST, distance_oracle.mean_sqdist(feats, feats[ROWS]), EXCLUDE + ROWS, distance=True)
    assert len(top_cosine[0]) == 10 and all_cosine[1].sum() == 18   # (the 20 entries less the excluded 200 and 8)
    for what, eng, _, _ in engines:
        listed = with_candidates(eng, LIST)
        _pair(listed.query_playlist_topn(ROWS, 10, exclude=EXCLUDE), top_cosine, f"{what}: playlist _candidates")
        _pair(listed.query_nearest_rows(ROWS, 10, exclude=EXCLUDE), top_distance, f"{what}: distance _candidates")
        candidate_scores_oracle.check(candidate_scores(eng, LIST, rows=ROWS, exclude=EXCLUDE), all_cosine, f"{what}: score playlist")
        candidate_scores_oracle.check(candidate_scores(eng, LIST, rows=ROWS, metric="distance", exclude=EXCLUDE), all_distance,
                                      f"{what}: score distance")
