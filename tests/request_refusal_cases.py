"""The fixed matrix of bad and cut request structs behind tests/golden/request_refusals.json: for each of the four kinds of request
(playlist, distance, any-of, Manhattan) the same cases through that kind's entry point that takes the ext, and for every case the
return code and the WHOLE text of the handle's last error.  tools/record_request_refusals.py wrote the fixture from these cases on the
CPU backend before the four conversions of csrc/playlist_request.h became one; tests/test_request_refusals_cpu.py and
tests/test_gpu_request_entry.py hold today's library to it.  Nothing here reads a message: a case is a struct, the text is the fixture's.

A case is (id, spec, conversion): `spec` says how the struct departs from the base request (two members by value, k = 2, top-5, nothing
else asked); `conversion` is true for the cases that the conversion itself or the first check behind it answers, with one text on
every handle type (the node handle and the CPU backend take an exclusion list and a catalogue of their own sizes, so the cases
after them are the CPU fixture's alone)."""
import ctypes
import json
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "request_refusals.json"
N_ROWS = 300
KINDS = ("playlist", "distance", "anyof", "manhattan")
ENTRY = {"playlist": "query_playlist_request_ext", "distance": "query_distance_request_ext", "anyof": "query_anyof_request",
         "manhattan": "query_manhattan_request"}
GOOD_SCALES = [2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0]
PQ_DIVERSE, PQ_CAPPED, PQ_PRIOR = 1, 2, 4


def catalogue() -> np.ndarray:
    return np.random.default_rng(24).random((N_ROWS, 12), dtype=np.float32)


def fixture() -> dict:
    return json.loads(FIXTURE.read_text())


def types(capi, kind):
    """(query struct, result struct) of a kind."""
    return {"playlist": (capi.PlaylistQuery, capi.PlaylistResult), "distance": (capi.DistanceQuery, capi.DistanceResult),
            "anyof": (capi.AnyOfQuery, capi.AnyOfResult), "manhattan": (capi.ManhattanQuery, capi.ManhattanResult)}[kind]


def field_ends(capi, kind) -> list:
    """Every size at which a struct of the kind ends where a field ends, the full size last."""
    query = types(capi, kind)[0]
    return [getattr(query, name).offset for name, _ in query._fields_[1:]] + [ctypes.sizeof(query)]


def cases(capi, kind) -> list:
    full = ctypes.sizeof(types(capi, kind)[0])
    out = []

    def add(name, conversion=True, **spec):
        out.append((name, spec, conversion))

    if kind == "playlist":
        add("flags unknown 8", flags=8)
        add("flags capped without diverse", flags=PQ_CAPPED)
        add("flags prior with size 84", flags=PQ_PRIOR, size=84)
    else:
        for flags in (1, 2, 4, 8, 0x80000000):
            add(f"flags {flags:#x}", flags=flags)
    add("members by value and by row", both=True)
    add("members neither by value nor by row", neither=True)
    for size in (0, 2, 6, 12, 47, 50, 63, full + 1, full + 8):
        add(f"size {size}", size=size)
    for end in field_ends(capi, kind):
        add(f"field end {end}", size=end)
    add("ext size 32", ext_size=32)
    add("rowset_mode 2 with a set", rowset="mine", rowset_mode=2)
    add("row set of another handle", rowset="foreign", rowset_mode=1)
    nan, negative = list(GOOD_SCALES), list(GOOD_SCALES)
    nan[3], negative[0] = float("nan"), -1.0
    for name, scales in (("good", GOOD_SCALES), ("nan", nan), ("negative", negative), ("all zero", [0.0] * 12)):
        add(f"scales {name}", scales=scales)
    if kind == "playlist":
        for name, flags in (("diverse", PQ_DIVERSE), ("capped", PQ_DIVERSE | PQ_CAPPED), ("prior", PQ_PRIOR)):
            add(f"scales with flags {name}", scales=GOOD_SCALES, flags=flags)
    for k in (0, 33):
        add(f"k {k}", False, k=k)
    for topn in (0, 1025):
        add(f"topn {topn}", False, topn=topn)
    add("null query", False, null_query=True)
    add("null result", False, null_result=True)
    add("null out_idx", False, null_idx=True)
    return out


def call(capi, lib, prefix, h, kind, spec, sets):
    """One case on handle `h` (`prefix`: "mi355rec_" or "mi355rec_sharded_"): (rc, the handle's whole last error; "" where rc is OK).
    `sets`: {"mine": a row set of h, "foreign": one of another handle}, as pointers."""
    Query, Result = types(capi, kind)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    members = np.ascontiguousarray(np.linspace(0.05, 0.95, 40 * 12, dtype=np.float32).reshape(40, 12))
    rows = np.asarray([1, 2], np.int64)
    q = Query()
    q.size = spec.get("size", ctypes.sizeof(Query))
    q.flags = spec.get("flags", 0)
    if not spec.get("neither"):
        q.members = ptr(members)
    if spec.get("both"):
        q.rows = ptr(rows)
    q.k, q.topn = spec.get("k", 2), spec.get("topn", 5)
    if kind == "playlist":
        q.lambda_, q.pool, q.max_per_group, q.prior_weight = 0.5, 8, 1, 0.25
    n_out = max(q.topn, 1)
    idx, val, member = np.zeros(n_out, np.int64), np.zeros(n_out, np.float32), np.zeros(n_out, np.int32)
    count = ctypes.c_int(0)
    res = Result()
    res.out_idx = None if spec.get("null_idx") else ptr(idx)
    setattr(res, "out_distance" if kind in ("distance", "manhattan") else "out_score", ptr(val))
    if kind == "anyof":
        res.out_member = ptr(member)
    res.out_count = ctypes.pointer(count)
    ext = None
    if any(key in spec for key in ("ext_size", "rowset", "scales")):
        scales = np.asarray(spec["scales"], np.float32) if "scales" in spec else None
        ext = capi.RequestExt(spec.get("ext_size", ctypes.sizeof(capi.RequestExt)), spec.get("rowset_mode", 0),
                              ptr(scales) if scales is not None else None, sets[spec["rowset"]] if "rowset" in spec else None)
    rc = getattr(lib, prefix + ENTRY[kind])(h, None if spec.get("null_query") else ctypes.byref(q), ctypes.byref(ext) if ext is not None else None,
                                            None if spec.get("null_result") else ctypes.byref(res))
    if rc == capi.OK:
        return rc, ""
    return rc, getattr(lib, prefix + "last_error")(h).decode()


def run(capi, lib, prefix, h, kind, sets, conversion_only=False) -> dict:
    """{case id: [rc, text]} of a kind on one handle."""
    return {name: list(call(capi, lib, prefix, h, kind, spec, sets)) for name, spec, conversion in cases(capi, kind)
            if conversion or not conversion_only}
