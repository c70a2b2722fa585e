"""One stream of single queries whose consecutive calls differ in everything a streamed launch is assembled from: how
the query is given (a catalogue row, 12 floats by value, a device pointer), topn (1, 10, and 700 — above the 640 whose
merge still rides in the next fp32 launch, so that merge takes a launch of its own) and, after the fourth call, the
kind of rows scanned (mi355rec_set_replica switches between the fp32 rows and the 8-bit replica under the running
stream, which costs the next query a sample launch of its own).

Two uniform catalogues, the smallest at which the launches have all their parts:
  70 000 rows     an 8-bit replica launch has seed riders and a neighbourhood workgroup from 16 tiles of 2048 rows
                  (plan_replica: grid >= 16, and the riders are capped at grid / 8 — 35 tiles give 4 of them);
  2 500 000 rows  the fp32 launch has seed riders from 2 M rows and a full grid (plan_grid).

Every key list against the CPU oracle, ids and score bits; the route counters show that both kinds were crossed.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from spotify_recommender_amd import capi
from tests.parity import assert_topn_matches

pytestmark = pytest.mark.gpu

TOPNS = (1, 10, 700)
FORMS = ("row", "value", "pointer")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def Engine(torch_cuda):
    from spotify_recommender_amd.engine import CosineEngine
    return CosineEngine


@pytest.mark.parametrize("n, first, second", [(70_000, capi.REPLICA_OFF, capi.REPLICA_ON),
                                              (2_500_000, capi.REPLICA_ON, capi.REPLICA_OFF)],
                         ids=["70k-off-to-on", "2.5M-on-to-off"])
def test_stream_of_mixed_forms_topns_and_kinds(Engine, torch_cuda, n, first, second):
    torch = torch_cuda
    from spotify_recommender_amd.engine import unpack_keys
    rng = np.random.default_rng(n)
    f = rng.random((n, 12), dtype=np.float32)
    rows = rng.integers(0, n, size=9).tolist()
    rows[0], rows[3] = n - 1, 0
    vecs = rng.random((9, 12), dtype=np.float32)
    vecs_dev = torch.from_numpy(vecs).to("cuda")
    # the forms cycle, and the topn cycle is shifted by one each round: every (form, topn) pair occurs once
    plan = [(FORMS[i % 3], TOPNS[(i + i // 3) % 3]) for i in range(9)]
    outs = [torch.zeros(t, dtype=torch.int64, device="cuda") for _, t in plan]
    torch.cuda.synchronize()
    with Engine(f) as eng:
        eng.set_replica(first)
        before = eng.stats()
        sp = eng._stream_ptr(None)
        for i, (form, topn) in enumerate(plan):
            if i == 4:
                eng.set_replica(second)
            if form == "row":
                eng.enqueue_row_keys_streamed(rows[i], topn, outs[i])
            elif form == "value":
                eng.enqueue_query_keys_streamed(vecs[i], -1, topn, outs[i])
            else:
                capi.check(eng._lib.mi355rec_enqueue_ptr_keys_streamed(
                    eng._h, ctypes.c_void_p(vecs_dev[i].data_ptr()), -1, topn, ctypes.c_void_p(outs[i].data_ptr()), sp), eng._h)
        eng.enqueue_flush()
        torch.cuda.synchronize()
        after = eng.stats()
    for i, (form, topn) in enumerate(plan):
        q, ex = (f[rows[i]], rows[i]) if form == "row" else (vecs[i], -1)
        want = oracle.scores(f, np.ascontiguousarray(q), threads=0)
        idx, sc = unpack_keys(outs[i].cpu().numpy())
        try:
            assert_topn_matches(idx, sc, want, ex, topn, ref_idx=oracle.topn_heap(want, ex, topn))
        except AssertionError as e:
            raise AssertionError(f"query {i} ({form}, topn {topn}): {e}") from e
    # four launches over the first kind of rows, five over the second
    fp32, q8 = after.route_fp32 - before.route_fp32, after.route_q8 - before.route_q8
    assert (fp32, q8) == ((4, 5) if first == capi.REPLICA_OFF else (5, 4)), (fp32, q8)
