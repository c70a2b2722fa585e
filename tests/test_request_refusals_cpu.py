"""The request structs' refusals on a host without a GPU, WHOLE texts and return codes: every case of tests/request_refusal_cases.py
(bad flags, members both ways and neither, every cut size and every field end, the ext's size and mode, a foreign row set, feature
scales with each kind, k, topn and null pointers) through the node handle's entry point of each of the four kinds, on the CPU
backend, against tests/golden/request_refusals.json — recorded (tools/record_request_refusals.py) while each kind still had its
own copy of the conversion.  The other tests look for substrings; this one pins every byte, the noun and its article included."""
import pytest

from tests import request_refusal_cases as cases


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")


@pytest.fixture(scope="module")
def handles(engine_lib):
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    feats = cases.catalogue()
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd, NodeEngine(feats[:50], placement=capi.PLACEMENT_AUTO) as other:
        assert nd.placement() == capi.PLACEMENT_CPU
        with nd.row_set([1, 2]) as mine, other.row_set([1, 2]) as foreign:
            yield nd, {"mine": mine._ptr(), "foreign": foreign._ptr()}


@pytest.mark.parametrize("kind", cases.KINDS)
def test_every_refusal_is_the_fixture(handles, kind):
    from spotify_recommender_amd import capi
    nd, sets = handles
    want = cases.fixture()[kind]
    got = cases.run(capi, nd._lib, "mi355rec_sharded_", nd._h, kind, sets)
    assert list(got) == list(want), "the matrix and the fixture name other cases: record again only if a message is meant to change"
    for name in want:
        assert got[name] == want[name], (kind, name)


def test_the_matrix_is_the_issue(engine_lib):
    """The fixture holds what it was specified to hold: per kind every listed size, every field end, and refusals that differ between
    the metric kinds in the noun alone."""
    from spotify_recommender_amd import capi
    fx = cases.fixture()
    for kind in cases.KINDS:
        full = cases.field_ends(capi, kind)[-1]
        for size in (0, 2, 6, 12, 47, 50, 63, full + 1, full + 8):
            assert fx[kind][f"size {size}"][0] == capi.ERR_INVALID_ARG and f"of size {size}: not the end of a field" in fx[kind][f"size {size}"][1]
        assert all(f"field end {e}" in fx[kind] for e in cases.field_ends(capi, kind))
        assert fx[kind][f"field end {full}"] == [capi.OK, ""]
    nouns = {"distance": ("a distance", "distance"), "anyof": ("an any-of", "any-of"), "manhattan": ("a manhattan", "manhattan")}
    for name, (rc, text) in fx["distance"].items():
        if name.startswith("scales"):
            continue   # (the distance request serves scales, the other two refuse them)
        for kind in ("anyof", "manhattan"):
            same = text.replace(nouns["distance"][0], nouns[kind][0]).replace(nouns["distance"][1], nouns[kind][1])
            assert fx[kind][name] == [rc, same], (kind, name)
