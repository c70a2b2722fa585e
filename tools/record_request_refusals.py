"""Records tests/golden/request_refusals.json: for each kind of request (playlist, distance, any-of, Manhattan) the return code and
the whole mi355rec_sharded_last_error text of every case of tests/request_refusal_cases.py, on the CPU backend (run it on a host
without a GPU) with a 300-row catalogue.  The committed fixture was recorded before the four struct conversions of
csrc/playlist_request.h became one; record again only when a message is MEANT to change, and say so in the commit.

    python tools/record_request_refusals.py [--out tests/golden/request_refusals.json]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def record() -> dict:
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import NodeEngine
    from tests import request_refusal_cases as cases
    feats = cases.catalogue()
    with NodeEngine(feats, placement=capi.PLACEMENT_AUTO) as nd, NodeEngine(feats[:50], placement=capi.PLACEMENT_AUTO) as other:
        if nd.placement() != capi.PLACEMENT_CPU:
            raise SystemExit("a GPU is visible: the fixture is the CPU backend's")
        with nd.row_set([1, 2]) as mine, other.row_set([1, 2]) as foreign:
            sets = {"mine": mine._ptr(), "foreign": foreign._ptr()}
            return {kind: cases.run(capi, nd._lib, "mi355rec_sharded_", nd._h, kind, sets) for kind in cases.KINDS}


def main():
    from tests.request_refusal_cases import FIXTURE
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(FIXTURE))
    a = ap.parse_args()
    first, second = record(), record()
    if first != second:
        raise SystemExit("two recordings differ: the texts are not deterministic")
    Path(a.out).write_text(json.dumps(first, indent=1) + "\n")
    print(f"{a.out}: {sum(len(v) for v in first.values())} cases")


if __name__ == "__main__":
    main()
