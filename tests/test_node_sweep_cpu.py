"""The node-handle sweep's case definitions, checked where no GPU is (tests/node_sweep_cases.py; the GPU leg is
tests/test_gpu_node_sweep.py): that the geometry list still covers what it claims, that the request matrix pushes a merge
over shards where it can go wrong (answers that span shards, lists shorter than topn, tied pairs across an edge), that at most
a quarter of the cases expect nothing, and that every case's expectation is what the product's CPU backend returns.

The CPU backend (csrc/cpu_backend.cpp) does NOT shard: it holds the whole catalogue behind the node handle.  So the last test
validates the cases and the oracles' composition (one exclusion list per request), and says nothing about the node layer itself:
merge_over_shards, diverse_over_shards, ShardLists and the per-shard slices run only on the MI355X (the merge's own arithmetic,
csrc/shard_merge.h, is checked without one by tests/test_shard_merge_cpu.py)."""
import numpy as np
import pytest

from tests import node_sweep_cases as cases


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


def test_the_geometries_cover_every_bit_phase_and_shard_size():
    """From the shard-bounds rule alone: the non-empty shards start at every lo % 8 and at all 32 values of lo % 32; shards of 0,
    1, 4 and 5 rows, one below each of top-10 / top-100 / top-1024, and the 64-shard case are there."""
    los, sizes = [], set()
    for n, g in cases.GEOMETRIES:
        b = cases.bounds(n, g)
        assert b[0][0] == 0 and b[-1][1] == n and all(b[r][1] == b[r + 1][0] for r in range(g - 1))
        los += [lo for lo, hi in b if hi > lo]
        sizes |= {hi - lo for lo, hi in b}
    assert {lo % 8 for lo in los} == set(range(8))
    assert {lo % 32 for lo in los} == set(range(32))
    assert {0, 1, 4, 5} <= sizes
    for topn in (10, 100, 1024):
        assert any(1 < s < topn for s in sizes), topn
    assert cases.WIDE in cases.GEOMETRIES and cases.WIDE[1] == 64
    assert set(cases.EMBED_GEOMETRIES) <= set(cases.GEOMETRIES) and {g for _, g in cases.ALTERNATE} <= {g for _, g in cases.GEOMETRIES}


@pytest.mark.parametrize("n, g, variant", cases.CATALOGUES)
def test_the_catalogue_is_what_the_merge_can_get_wrong(n, g, variant):
    cat = cases.catalogue(n, g, variant)
    f = cat.feats
    edges = [cat.bounds[s][0] for s in cat.nonempty[1:]]
    if variant == "tied":
        assert [b for _, b in cat.pairs] == edges                            # both sides of EVERY edge
    for a, b in cat.pairs:
        assert cat.shard[a] + 1 <= cat.shard[b] and np.array_equal(f[a].view(np.uint32), f[b].view(np.uint32))
    paired = {r for p in cat.pairs for r in p}
    assert not paired & set(cat.hostile) and (n < 259 or len(cat.hostile) == 6)
    # labels: one lives in a single shard, one is absent from a shard, all of them together cover every labelled row
    assert np.unique(cat.shard[cat.labels == cases.L_ONE]).size == 1
    if len(cat.nonempty) > 1:
        assert set(cat.shard[cat.labels == cases.L_ABSENT]) < set(cat.nonempty)
    assert not np.any(cat.labels == cases.L_NONE)
    # priors in [-1, 1], the largest on a one-row shard where there is one; group 0 on every shard
    assert np.all(np.abs(cat.priors) <= 1) and cat.priors.max() == 1.0
    if 1 in cat.sizes:
        assert cat.sizes[cat.shard[int(np.argmax(cat.priors))]] == 1
    assert set(cat.shard[cat.groups == 0]) == set(cat.nonempty)
    # the standard request: the short shard's own rows lead it, the starved shard has none of its top-10
    plain10 = next(c for c in cases.matrix(n, g, variant) if c.kind == "cosine" and c.what == "plain by value, top-10")
    if cat.short is not None and cat.sizes[cat.short] >= 2 and variant == "tied" and max(cat.sizes) > 2:
        lo, hi = cat.bounds[cat.short]
        own = [r for r in range(lo + 1, min(hi, lo + 9)) if f[r, 11] == np.float32(0.25)]   # (not the neighbour's copy, not a FEW row)
        calm = [r for r in plain10.ids.tolist() if r not in cat.hostile]       # (an infinite feature scores 1.0: the oracle's clamp)
        assert set(calm[:min(len(calm), len(own))]) <= set(own)
    if cat.starved is not None and n - cat.sizes[cat.starved] >= 10 and max(cat.sizes) > 2:
        lo, hi = cat.bounds[cat.starved]
        assert not set(plain10.ids.tolist()) & set(range(lo + 1, hi))          # (its first row is the copy of its neighbour's last)


@pytest.mark.parametrize("n, g, variant", cases.CATALOGUES)
def test_every_kind_pushes_the_merge_past_a_shards_end(n, g, variant):
    """Per geometry and kind, from the oracle alone: an answer from two shards at least, an answer that holds every admissible
    row of some shard (a list shorter than topn), and every admissible tied pair in id order."""
    cat = cases.catalogue(n, g, variant)
    todo = cases.matrix(n, g, variant)
    kinds = cases.WIDE_KINDS if (n, g) == cases.WIDE else cases.KINDS
    assert {c.kind for c in todo} == set(kinds)
    for kind in kinds:
        mine = [c for c in todo if c.kind == kind]
        could_span = [c for c in mine if c.get("topn", 0) >= 2 and np.unique(cat.shard[np.flatnonzero(c.adm)]).size >= 2]
        if len(cat.nonempty) >= 2 and could_span:
            assert any(cases.spans_shards(cat, c) for c in mine), f"{kind}: no answer from two shards"
        if any(c.ids.size for c in mine):
            assert any(cases.takes_a_whole_shard(cat, c) for c in mine), f"{kind}: no answer takes all of a shard's admissible rows"
        for c in mine:
            assert cases.tied_pairs_in_order(cat, c), f"{kind}: {c.what}: a tied pair out of id order"
    if (n, g) != cases.WIDE:   # any-of attribution differs between shards, and a tie between members goes to the lower index
        a = next(c for c in todo if c.kind == "anyof" and c.what.startswith("by value") and c.get("topn") == 1024)
        assert 2 not in a.want[2].tolist() and (n < 13 or len(set(a.want[2].tolist())) >= 2)
    bounded = [c for c in todo if c.kind == "bounded" and c.get("metric") == "cosine" and c.get("where") is None]
    assert any(c.want[2] == 0 for c in bounded) and any(c.want[2] > 0 for c in bounded)
    if cat.short is not None and cat.sizes[cat.short] >= 3 and variant == "tied":
        assert any(c.want[2] > 0 and np.unique(cat.shard[np.flatnonzero(c.adm)]).size == 1 for c in bounded), "no floor only one shard meets"


def test_at_most_a_quarter_of_the_cases_expect_an_empty_answer():
    """Over every case of the sweep, from the oracles' answers (no call is made here)."""
    empty, total = cases.empty_share()
    print(f"{empty} of {total} node-sweep cases expect an empty answer ({100.0 * empty / total:.1f} %)")
    per_kind = {k: sum(1 for n, g, v in cases.CATALOGUES for c in cases.matrix(n, g, v) if c.kind == k) for k in cases.KINDS}
    print("cases per kind:", per_kind)
    assert total > 0 and 4 * empty <= total, f"{empty} of {total} cases expect an empty answer: more than a quarter"


@pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")
@pytest.mark.parametrize("n, g, variant", cases.CATALOGUES)
def test_the_cases_match_the_cpu_backend(engine_lib, n, g, variant):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    cat = cases.catalogue(n, g, variant)
    with NodeEngine(cat.feats, placement=capi.PLACEMENT_AUTO) as nd:
        assert nd.placement() == capi.PLACEMENT_CPU
        nd.set_labels(cat.labels)
        nd.set_priors(cat.priors)
        nd.set_groups(cat.groups)
        for c in cases.matrix(n, g, variant):
            cases.check(c, cases.run(nd, c), f"n={n} over {g} [{variant}]")
        rows, new, after = cat.updated()
        nd.update_rows(rows, new)
        for c in cases.request_matrix(after, short=True):
            cases.check(c, cases.run(nd, c), f"n={n} over {g} [{variant}] after update_rows")
