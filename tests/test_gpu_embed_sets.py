"""RESTRICTED EMBEDDING REQUESTS on the GPU (include/mi355rec_embed_sets.h, csrc/embed_sets.hip.h):
embed_sets_scan_kernel's answers, three storages, bit for bit against tests/embed_oracle.py with the ids of `seen` and the
complement of `only` excluded — at the sizes where the kernel can go wrong (the word edges 31 / 32 / 33 and 63 / 64 / 65, one
tile more or less, several workgroups, a full grid), with the sets that can go wrong (empty, every row, one bit at either
end, rows 31 and 32 alone, every other row, random ones, the whole unrestricted answer as `seen`, both sets at once, only
inside seen); the identities against the first and the third companion on the same engine; the tile skip, counted; the
steady state at a million rows; a row base; two tables on one handle; add between queries; the calls answered without a
launch.  Hostile means values, never addresses."""
import numpy as np
import pytest

from tests import embed_cases as ec
from tests import embed_oracle as eo
from tests import embed_sets_cases as sc

pytestmark = pytest.mark.gpu
F32 = np.float32


def _table(eng, given):
    from spotify_recommender_amd.embed_sets import RestrictedEmbeddingTable
    return RestrictedEmbeddingTable(eng, given)


def _sizes(group, d, storage):
    if group == "edges":
        return [1, 2, 31, 32, 33, 63, 64, 65]
    if group == "tile":
        from spotify_recommender_amd import CosineEngine
        with CosineEngine(np.ones((1, 12), F32)) as eng, _table(eng, sc.given(1, d, storage)[1]) as tab:
            t = tab.info()["tile_rows"]   # asked of the library (a one-row table)
        assert t == sc.tile_rows(d, storage)
        return [t - 1, t, t + 1, 2 * t + 1]
    return [4097] if group == "blocks" else [65537]


@pytest.mark.parametrize("storage", sc.STORAGES)
@pytest.mark.parametrize("group", ["edges", "tile", "blocks", "many"])
@pytest.mark.parametrize("d", sc.DIMS)
def test_restricted_scan_matches_the_oracle(d, group, storage):
    from spotify_recommender_amd import CosineEngine, capi
    code = {"f32": capi.EMBED_SETS_FP32, "fp16": capi.EMBED_HALF_FP16, "bf16": capi.EMBED_HALF_BF16}[storage]
    for n in _sizes(group, d, storage):
        feats, given = sc.given(n, d, storage)
        sets = sc.row_sets(n)
        with CosineEngine(feats) as eng, _table(eng, given) as tab:
            info = tab.info()
            assert (info["rows"], info["dim"], info["shards"], info["storage"]) == (n, d, 1, code) and info["grid"] >= 1
            assert info["tile_rows"] == sc.tile_rows(d, storage)
            n_tiles = -(-n // info["tile_rows"])
            table = tab.widened()
            handles = {name: tab.rowset(rows) for name, rows in sets.items()}
            for name, rows in sets.items():
                assert handles[name].count == len(rows), name
            # both sets at once, with an overlap (rows of `half` that `alternate` also holds are left out); only inside seen
            superset = tab.rowset(np.concatenate([sets["half"], sets["percent"]]))
            asked = skipped = with_audio = 0
            for i, req in enumerate(ec.requests(n, d)):
                v = sc.values(feats, table, req)
                what = f"{storage} n={n} d={d} request {i}"
                plain = sc.check(tab, v, req, what + ", no sets")
                cases = [(None, None)]
                for name in sets:
                    sc.check(tab, v, req, f"{what}, only={name}", only=sets[name], only_set=handles[name])
                    sc.check(tab, v, req, f"{what}, seen={name}", seen=sets[name], seen_set=handles[name])
                    cases += [(None, sets[name]), (sets[name], None)]
                # the whole unrestricted answer as `seen`: the next page shares no id with it
                with tab.rowset(plain) as page:
                    nxt = sc.check(tab, v, req, what + ", seen = the plain answer", seen=plain, seen_set=page)
                    assert not set(nxt.tolist()) & set(plain.tolist())
                    cases.append((plain, None))
                sc.check(tab, v, req, what + ", only=half seen=alternate", seen=sets["alternate"], only=sets["half"],
                         seen_set=handles["alternate"], only_set=handles["half"])
                cases.append((sets["alternate"], sets["half"]))
                got = sc.check(tab, v, req, what + ", only inside seen", seen=np.concatenate([sets["half"], sets["percent"]]),
                               only=sets["percent"], seen_set=superset, only_set=handles["percent"])
                assert got.size == 0
                cases.append((np.concatenate([sets["half"], sets["percent"]]), sets["percent"]))
                nothing = sum(1 for seen, only in cases if sc.answers_nothing(n, seen, only))
                asked += len(cases)
                skipped += nothing
                with_audio += (len(cases) - nothing) * (req.get("audio_weight", 0.0) != 0.0)
            after = tab.info()
            assert after["queries"] == asked and after["launches_skipped"] == skipped
            assert after["tiles_total"] == (asked - skipped) * n_tiles and 0 < after["tiles_scored"] <= after["tiles_total"]
            assert after["scores_launches"] == with_audio   # (none with w_audio == 0, none for a call without a launch)
            superset.close()
            for h in handles.values():
                h.close()


@pytest.mark.parametrize("storage", sc.STORAGES)
@pytest.mark.parametrize("n,d", [(33, 16), (4099, 32), (3001, 128)])
def test_the_identities_against_the_other_companions(n, d, storage):
    """No sets, `only` of every row and an empty `seen`: the plain call's answer.  `seen` of at most 1024 rows: the plain call
    with the rows appended to exclude_global (where the list has room).  The count-0 cases."""
    from spotify_recommender_amd import CosineEngine
    from spotify_recommender_amd.embed import EmbeddingTable
    from spotify_recommender_amd.embed_half import HalfEmbeddingTable
    feats, given = sc.given(n, d, storage)
    sets = sc.row_sets(n)
    small = sets["percent"] if n >= 100 else sets["half"]
    with CosineEngine(feats) as eng, _table(eng, given) as tab:
        with (EmbeddingTable(eng, given) if storage == "f32" else HalfEmbeddingTable(eng, given)) as plain_tab:
            with tab.rowset(sets["all"]) as every, tab.rowset([]) as none, tab.rowset(small) as seen:
                appended = 0
                for i, req in enumerate(ec.requests(n, d)):
                    want = plain_tab.query(**req)
                    for kw in (dict(), dict(only=every), dict(seen=none), dict(only=every, seen=none)):
                        got = tab.query(**req, **kw)
                        assert got[0].tolist() == want[0].tolist() and np.array_equal(eo.bits(got[1]), eo.bits(want[1])), (storage, i, sorted(kw))
                    for kw in (dict(only=none), dict(seen=every), dict(only=seen, seen=seen), dict(only=seen, seen=every)):
                        assert tab.query(**req, **kw)[0].size == 0, (storage, i, sorted(kw))
                    excl = list(req.get("exclude", [])) + small.tolist()
                    if len(excl) + len(req.get("rows", [])) <= 1024:
                        want = plain_tab.query(**dict(req, exclude=excl))
                        got = tab.query(**req, seen=seen)
                        assert got[0].tolist() == want[0].tolist() and np.array_equal(eo.bits(got[1]), eo.bits(want[1])), (storage, i, "seen")
                        appended += 1
                assert appended >= 6


def _skip_table(n, d, storage, keep, seed):
    """A random table whose rows outside `keep` (local rows) hold inf and 3e38: a skipped tile scored by mistake would show."""
    rng = np.random.default_rng(seed)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    out = np.ones(n, bool)
    out[keep] = False
    hostile = np.nonzero(out)[0]
    table[hostile[0::2]] = np.inf
    table[hostile[1::2]] = F32(3e38)
    if storage == "f32":
        return feats, table
    from spotify_recommender_amd.embed_half import to_storage
    from tests import embed_half_cases as hc
    return feats, hc.as_given(to_storage(table, storage), storage)


@pytest.mark.parametrize("d,storage", [(64, "f32"), (16, "fp16")])
def test_tiles_without_an_admissible_row_are_not_scored(d, storage):
    """n = 8 tiles + 5 rows: tiles_scored grows by exactly the tiles that hold a row of `only AND NOT seen`."""
    from spotify_recommender_amd import CosineEngine
    t = sc.tile_rows(d, storage)
    n = 8 * t + 5
    rows = np.arange(n, dtype=np.int64)
    cases = [
        ("tile 3", rows[3 * t: 4 * t], None, 1),
        ("mid 2 to mid 4", rows[2 * t + t // 2: 4 * t + t // 2], None, 3),
        ("the last, partial tile", rows[8 * t:], None, 1),
        ("every second tile", rows[(rows // t) % 2 == 0], None, 5),
        ("mid 2 to mid 4, tile 3 seen", rows[2 * t + t // 2: 4 * t + t // 2], rows[3 * t: 4 * t], 2),
        ("one row of tile 0 and one of tile 7", np.array([t - 1, 7 * t], np.int64), None, 2),
    ]
    user = np.random.default_rng(4).standard_normal(d, dtype=F32)
    reqs = [dict(user=user, metric="cosine", embed_weight=1.0, topn=10),
            dict(rows=[0], metric="dot", embed_weight=-1.0, audio_weight=0.5, audio_row=1, topn=1024, exclude_rows=False)]
    for k, (what, only, seen, tiles) in enumerate(cases):
        keep = only if seen is None else np.setdiff1d(only, seen)
        feats, given = _skip_table(n, d, storage, np.concatenate([keep, [0]]), seed=k)
        with CosineEngine(feats) as eng, _table(eng, given) as tab:
            assert tab.info()["tile_rows"] == t and tab.info()["grid"] == 9
            table = tab.widened()
            with tab.rowset(only) as only_set, tab.rowset([] if seen is None else seen) as seen_set:
                for i, req in enumerate(reqs):
                    before = tab.info()
                    plain = {key: val for key, val in req.items() if key != "exclude_rows"}
                    v = sc.values(feats, table, plain)
                    ids, scores = sc.expected(v, dict(plain, rows=[]), seen, only)
                    gi, gs = tab.query(**req, only=only_set, seen=seen_set if seen is not None else None)
                    assert gi.tolist() == ids.tolist() and np.array_equal(eo.bits(gs), eo.bits(scores)), (what, i)
                    assert gi.size == min(req["topn"], int(np.isfinite(v[keep]).sum())) > 0, (what, i)
                    after = tab.info()
                    assert after["tiles_scored"] - before["tiles_scored"] == tiles, (what, i)
                    assert after["tiles_total"] - before["tiles_total"] == 9, (what, i)


@pytest.mark.parametrize("storage", ["f32", "fp16"])
def test_a_million_rows_steady_state(storage):
    """1 000 003 rows at d = 16: the grid is full and every workgroup takes several tiles.  A random half as `only`, top-10 and
    top-1024; one contiguous 1 / 114 of the rows (a genre of a catalogue grouped by genre): at most its tiles + 2 are scored."""
    from spotify_recommender_amd import CosineEngine
    n, d = 1_000_003, 16
    rng = np.random.default_rng(9)
    feats = rng.random((n, 12), dtype=F32)
    table = rng.standard_normal((n, d), dtype=F32)
    table[123_456] = table[7]
    feats[123_456] = feats[7]
    user = rng.standard_normal(d, dtype=F32)
    half = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)
    run = np.arange(400_001, 400_001 + n // 114, dtype=np.int64)
    given = table
    if storage != "f32":
        from spotify_recommender_amd.embed_half import to_storage
        from tests import embed_half_cases as hc
        given = hc.as_given(to_storage(table, storage), storage)
    with CosineEngine(feats) as eng, _table(eng, given) as tab:
        info = tab.info()
        t = info["tile_rows"]
        n_tiles = -(-n // t)
        assert info["grid"] > 64 and n_tiles >= 1.9 * info["grid"]
        wide = tab.widened()
        mask = np.zeros(n, bool)
        mask[half] = True
        with tab.rowset_from_mask(mask) as half_set, tab.rowset(run) as run_set:
            assert half_set.count == half.size and run_set.count == run.size
            req = dict(user=user, metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=7, topn=10, exclude=[7, 7, n + 1])
            v = sc.values(feats, wide, req)
            for topn in (10, 1024):
                sc.check(tab, v, dict(req, topn=topn), f"a random half, top-{topn}", only=half, only_set=half_set)
            before = tab.info()
            sc.check(tab, v, dict(req, topn=1024), "one contiguous run", only=run, only_set=run_set)
            after = tab.info()
            assert after["tiles_total"] - before["tiles_total"] == n_tiles
            assert 0 < after["tiles_scored"] - before["tiles_scored"] <= -(-run.size // t) + 2
            dot = dict(rows=[5, 6, 7], metric="dot", embed_weight=1.0, topn=1024)
            sc.check(tab, sc.values(feats, wide, dot), dot, "dot, the run without the half", only=run, seen=half, only_set=run_set, seen_set=half_set)


@pytest.mark.parametrize("storage", sc.STORAGES)
def test_a_shard_with_a_row_base(storage):
    """A single handle that is one shard of a larger catalogue: set ids are global (bit = id - row_base), ids of other shards
    match nothing."""
    from spotify_recommender_amd import CosineEngine
    n, d, base = 1500, 32, 1_000_000
    feats, given = sc.given(n, d, storage)
    sets = sc.row_sets(n)
    with CosineEngine(feats, row_base=base) as eng, _table(eng, given) as tab:
        table = tab.widened()
        foreign = np.array([7, 31, base - 1, base + n, base + n + 40, 2 ** 40], np.int64)
        with tab.rowset(np.concatenate([sets["half"] + base, foreign])) as half, tab.rowset(np.concatenate([foreign, sets["percent"] + base])) as pct, \
                tab.rowset(foreign) as none:
            assert (half.count, pct.count, none.count) == (sets["half"].size, sets["percent"].size, 0)
            req = dict(rows=[3, 4, 5], metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=10, topn=40, exclude=[base + 7, 7, base + n])
            v = sc.values(feats, table, req)
            sc.check(tab, v, req, "only", only=sets["half"], only_set=half, row_base=base)
            sc.check(tab, v, req, "seen", seen=sets["half"], seen_set=half, row_base=base)
            sc.check(tab, v, req, "both", seen=sets["percent"], only=sets["half"], seen_set=pct, only_set=half, row_base=base)
            sc.check(tab, v, req, "foreign ids alone: an empty seen", seen=[], seen_set=none, row_base=base)
            assert tab.query(**req, only=none)[0].size == 0


def test_two_tables_and_their_sets_on_one_handle():
    """Each table's buffers and sets are its own; a set of another table is refused; the engine still answers between them."""
    from spotify_recommender_amd import CosineEngine, capi
    n = 3001
    feats, t16 = sc.given(n, 16, "fp16")
    _, t128 = sc.given(n, 128, "f32", seed=3)
    sets = sc.row_sets(n)
    with CosineEngine(feats) as eng, _table(eng, t16) as a, _table(eng, t128) as b:
        with a.rowset(sets["half"]) as sa, b.rowset(sets["alternate"]) as sb:
            for i in range(3):   # alternately
                ra, rb = ec.requests(n, 16)[i], ec.requests(n, 128)[i]
                sc.check(a, sc.values(feats, a.widened(), ra), ra, f"fp16 table, request {i}", only=sets["half"], only_set=sa)
                sc.check(b, sc.values(feats, b.widened(), rb), rb, f"fp32 table, request {i}", seen=sets["alternate"], seen_set=sb)
            req = ec.requests(n, 16)[0]
            for kw in (dict(only=sb), dict(seen=sb), dict(only=sa, seen=sb)):
                with pytest.raises(capi.Mi355Error, match="row set of another table") as err:
                    a.query(**req, **kw)
                assert err.value.code == capi.ERR_INVALID_ARG
            sc.check(a, sc.values(feats, a.widened(), req), req, "after the refusals", seen=sets["half"], seen_set=sa)
        from oracle import oracle
        idx, _ = eng.query_row_topn(5, 10)
        assert idx.tolist() == oracle.topn_canonical(oracle.scores(feats, feats[5]), 5, 10)[0].tolist()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_add_is_seen_by_the_next_query_and_a_failed_add_by_none(storage):
    from spotify_recommender_amd import CosineEngine, capi
    n, d = 70_001, 16
    feats, given = sc.given(n, d, storage)
    req = dict(rows=[4, 9, 100], metric="cosine", embed_weight=0.05, audio_weight=1.0, audio_row=77, topn=50)
    with CosineEngine(feats) as eng, _table(eng, given) as tab:
        v = sc.values(feats, tab.widened(), req)
        with tab.rowset([]) as seen:
            listened = np.zeros(0, np.int64)
            for page in range(4):   # every page is added to the history: the next one shares nothing with it
                got = sc.check(tab, v, req, f"page {page}", seen=listened, seen_set=seen)
                assert got.size == 50 and not set(got.tolist()) & set(listened.tolist())
                seen.add(np.concatenate([got, got[:3], [n + 5]]))   # duplicates and a foreign id
                listened = np.concatenate([listened, got])
                assert seen.count == listened.size
            for bad, text in (([1, -1, 2], "negative id -1"),):
                with pytest.raises(capi.Mi355Error, match=text) as err:
                    seen.add(bad)
                assert err.value.code == capi.ERR_INVALID_ARG and seen.count == listened.size
            sc.check(tab, v, req, "after the failed add", seen=listened, seen_set=seen)
        with pytest.raises(capi.Mi355Error, match="negative id -7"):
            tab.rowset([3, -7])
        with pytest.raises(capi.Mi355Error, match=f"mask of {n - 1} bytes for a table of {n} rows"):
            tab.rowset_from_mask(np.ones(n - 1, bool))
        labels = np.arange(n) % 114
        with tab.rowset_from_mask(labels == 5) as genre:   # a label selection, made by the caller
            sc.check(tab, v, req, "a label selection", only=np.nonzero(labels == 5)[0], only_set=genre)


def test_calls_without_an_admissible_row_launch_nothing():
    """only empty, seen of every row, only inside seen: count 0, launches_skipped grows and no launch counter moves."""
    from spotify_recommender_amd import CosineEngine
    n, d = 5000, 64
    feats, given = sc.given(n, d, "f32")
    sets = sc.row_sets(n)
    req = dict(rows=[4, 9], metric="cosine", embed_weight=0.5, audio_weight=1.0, audio_row=3, topn=20)
    with CosineEngine(feats) as eng, _table(eng, given) as tab:
        with tab.rowset([]) as none, tab.rowset(sets["all"]) as every, tab.rowset(sets["percent"]) as pct, tab.rowset(sets["percent"]) as grown:
            grown.add(sets["half"])
            v = sc.values(feats, tab.widened(), req)
            sc.check(tab, v, req, "a launch first", only=sets["percent"], only_set=pct)
            before = tab.info()
            assert before["launches_skipped"] == 0 and before["tiles_total"] > 0 and before["scores_launches"] == 1
            kws = [dict(only=none), dict(seen=every), dict(only=pct, seen=grown), dict(only=pct, seen=every), dict(only=none, seen=none)]
            for k, kw in enumerate(kws):
                ids, scores = tab.query(**req, **kw)
                assert ids.size == 0 and scores.size == 0
                after = tab.info()
                assert after["launches_skipped"] == k + 1 and after["queries"] == before["queries"] + k + 1
                for name in ("tiles_total", "tiles_scored", "scores_launches", "device_bytes"):
                    assert after[name] == before[name], name
            # an invalid request is still refused, whatever its sets
            from spotify_recommender_amd import capi
            with pytest.raises(capi.Mi355Error, match=r"topn 1025 out of \[1, 1024\]"):
                tab.query(**dict(req, topn=1025), only=none)
            # grown holds pct: the reverse is no subset, and it launches
            sc.check(tab, v, req, "seen inside only", only=np.union1d(sets["half"], sets["percent"]), seen=sets["percent"], only_set=grown, seen_set=pct)
            assert tab.info()["launches_skipped"] == len(kws)
