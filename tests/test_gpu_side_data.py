"""The per-row side data of a handle (labels, groups, priors: csrc/engine_state.hip.h RowSide, one owner) on the MI355X, one
body for the three attributes: shared with a lane that outlives its parent, refused on a handle with lanes, set / replaced /
dropped on a single handle and through the node handle whose replicas {0, 0} are lanes on one device, and all three freed
once whatever the order the members of a group are destroyed in.  1 000 seeded random rows (no ties); every answer bit for
bit against the oracle (ids, score bits, mmr bits, count, P'; the raw calls check the padding)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.labels_oracle import expected_from_scores as expected_labels
from tests.playlist_labels_oracle import expected_diverse, expected_scored, scores_of
from tests.prior_oracle import expected_prior, request_call

pytestmark = pytest.mark.gpu

N = 1000
Q_ROW, WANTED = 7, [1, 3]           # the filtered query
MEMBERS = [11, 500, 999]            # the playlist requests
LAM, POOL, CAP, BETA = 0.7, 64, 1, 1.0


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _is_node(obj):
    from spotify_recommender_amd.engine import NodeEngine
    return isinstance(obj, NodeEngine)


def _message(obj):
    fn = obj._lib.mi355rec_sharded_last_error if _is_node(obj) else obj._lib.mi355rec_last_error
    return (fn(obj._h) or b"").decode()


def _ask(kind, obj):
    """The attribute's query through a handle or a node handle: (rc, ids, scores, mmr, pool_rows), cut at the count."""
    from spotify_recommender_amd import capi
    prefix = "mi355rec_sharded_" if _is_node(obj) else "mi355rec_"
    if kind == "labels":
        topn = 40
        idx, score, count = np.full(topn, -7, np.int64), np.full(topn, 9.0, np.float32), ctypes.c_int(-7)
        want = np.asarray(WANTED, np.int32)
        rc = getattr(obj._lib, prefix + "query_row_topn_labels")(obj._h, Q_ROW, _ptr(want), want.size, topn, _ptr(idx), _ptr(score), ctypes.byref(count))
        c = max(count.value, 0)
        if rc == 0:
            assert np.all(idx[c:] == -1) and not score[c:].view(np.uint32).any(), "padding"
        return rc, idx[:c].copy(), score[:c].copy(), np.zeros(c, np.float32), 0
    fn = getattr(obj._lib, prefix + "query_playlist_request")
    if kind == "groups":
        return request_call(capi, fn, obj._h, rows=MEMBERS, topn=20, lam=LAM, pool=POOL, max_per_group=CAP)
    return request_call(capi, fn, obj._h, rows=MEMBERS, topn=50, prior_weight=BETA)


@pytest.fixture(scope="module")
def world(engine_lib):
    """(feats, {kind: (values A, values B)}, {kind: (expected with A, expected with B)}): computed once, never modified."""
    feats = np.ascontiguousarray(oracle.mt19937_uniform(1000, N))
    rng = np.random.default_rng(10)
    rows = np.arange(N)
    lab = [rng.integers(0, 6, size=N).astype(np.int32) for _ in range(2)]
    lab[0][rng.random(N) < 0.05] = -1
    values = {"labels": tuple(lab),
              "groups": ((rows % 7).astype(np.int32), (rows // 3).astype(np.int32)),
              "priors": ((rng.random(N, dtype=np.float32) * 2 - 1).astype(np.float32), rng.random(N, dtype=np.float32))}
    s_row = oracle.scores(feats, feats[Q_ROW])
    s_pl = scores_of(feats, feats[MEMBERS])
    pool = expected_scored(s_pl, feats, None, None, MEMBERS, POOL)
    want = {"labels": tuple(expected_labels(s_row, v, Q_ROW, WANTED, 40) for v in values["labels"]),
            "groups": tuple(expected_diverse(pool, feats, LAM, 20, v, CAP) for v in values["groups"]),
            "priors": tuple(expected_prior(s_pl, v, BETA, feats, None, None, MEMBERS, 50) for v in values["priors"])}
    for kind in want:   # replacing must change the answer, or the steps below prove nothing
        assert want[kind][0][0].tolist() != want[kind][1][0].tolist(), kind
    return feats, values, want


def _answers(kind, obj, want, what):
    rc, ids, sc, mmr, pool_rows = _ask(kind, obj)
    assert rc == 0, f"{what}: rc {rc}: {_message(obj)}"
    assert ids.tolist() == np.asarray(want[0]).tolist(), f"{what}: ids differ"
    assert np.array_equal(sc.view(np.uint32), (np.asarray(want[1], np.float32) + np.float32(0)).view(np.uint32)), f"{what}: scores differ"
    if kind == "groups":
        assert np.array_equal(mmr.view(np.uint32), np.asarray(want[2], np.float32).view(np.uint32)), f"{what}: mmr differs"
        assert pool_rows == POOL, f"{what}: pool_rows {pool_rows}"


def _refuses(call, obj, message, exact=True):
    from spotify_recommender_amd import capi
    with pytest.raises(capi.Mi355Error) as err:
        call()
    assert err.value.code == capi.ERR_INVALID_ARG
    got = _message(obj)
    assert got == message if exact else message in got, got


def _has_none(kind, obj, exact=True):
    from spotify_recommender_amd import capi
    rc = _ask(kind, obj)[0]
    assert rc == capi.ERR_INVALID_ARG, rc
    got = _message(obj)
    if exact:
        assert got == f"this handle has no {kind} (mi355rec_set_{kind})", got
    else:   # (the node handle names its own setter, or passes a shard's message on)
        assert f"this handle has no {kind} (mi355rec_" in got, got


@pytest.mark.parametrize("kind", ["labels", "groups", "priors"])
def test_shared_refused_replaced_dropped(world, kind):
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from spotify_recommender_amd import CosineEngine, capi
    from spotify_recommender_amd.engine import NodeEngine
    feats, values, want = world
    a, b = values[kind]
    has_lanes = f"the handle has lanes: set the {kind} before the first lane is made"

    def setter(obj):
        return getattr(obj, "set_" + kind)

    # a lane made after the setter shares the data, and keeps it when the parent goes first
    eng = CosineEngine(feats)
    setter(eng)(a)
    lane = eng.lane()
    try:
        _refuses(lambda: setter(eng)(b), eng, has_lanes)
        _refuses(lambda: setter(eng)(None), eng, has_lanes)
        eng.close()
        _answers(kind, lane, want[kind][0], f"{kind}: the lane after its parent")
        _refuses(lambda: setter(lane)(b), lane, has_lanes)
        _answers(kind, lane, want[kind][0], f"{kind}: the lane after the refused setter")
    finally:
        eng.close()
        lane.close()

    # set, replace, drop on a fresh handle
    with CosineEngine(feats) as eng:
        _has_none(kind, eng)
        setter(eng)(a)
        _answers(kind, eng, want[kind][0], f"{kind}: set")
        setter(eng)(b)
        _answers(kind, eng, want[kind][1], f"{kind}: replaced")
        setter(eng)(None)
        _has_none(kind, eng)
        setter(eng)(a)
        _answers(kind, eng, want[kind][0], f"{kind}: set again after the drop")

    # the same through the node handle whose two replicas are lanes on one device: it replaces under its own lanes, and
    # every replica (they take turns) gives the single handle's answer
    with NodeEngine(feats, devices=[0, 0], placement=capi.PLACEMENT_REPLICATED) as node:
        for step, (v, w) in enumerate(((a, want[kind][0]), (b, want[kind][1]), (None, None), (a, want[kind][0]))):
            setter(node)(v)
            for turn in range(3):
                if v is None:
                    _has_none(kind, node, exact=False)
                else:
                    _answers(kind, node, w, f"{kind}: node step {step}, call {turn}")


@pytest.mark.parametrize("order", ["parent-lane-lane", "lane-parent-lane"])
def test_all_three_are_freed_once_in_any_order(world, order):
    import torch  # noqa: F401
    from spotify_recommender_amd import CosineEngine, capi
    feats, values, want = world
    lib = capi.lib()
    eng = CosineEngine(feats)
    members = [eng]
    try:
        for kind in ("labels", "groups", "priors"):
            getattr(eng, "set_" + kind)(values[kind][0])
        members += [eng.lane(), eng.lane()]
        for m, name in zip(members, ("parent", "lane 1", "lane 2")):
            for kind in ("labels", "groups", "priors"):
                _answers(kind, m, want[kind][0], f"{kind} on the {name}")
        before = lib.mi355rec_last_global_error()
        for i in ((0, 1, 2) if order == "parent-lane-lane" else (1, 0, 2)):
            members[i].close()
            for m in members:   # whoever is left still answers from the group's data
                if m._h:
                    _answers("groups", m, want["groups"][0], f"after closing member {i} ({order})")
        # the runtime is sound afterwards (every launch checks hipGetLastError) and no call has reported an error since
        with CosineEngine(feats) as fresh:
            fresh.set_priors(values["priors"][1])
            _answers("priors", fresh, want["priors"][1], f"a fresh handle after {order}")
        after = lib.mi355rec_last_global_error()
        assert after == before, after
    finally:
        for m in members:
            m.close()
