"""Lists, tables and the LIST-OCCUPANCY MODEL of the candidate gather's STEADY STATE (csrc/embed_cand.hip.h's
embed_cand_kernel, selecting form): one workgroup of the gather is fed several full tiles of rows that all beat its
threshold, so the loop's three-deep carry (cur_r / next_r / far_r, cur_e, cur_s), its own mid-loop compaction, its threshold
and its LDS exclusion search are all in play.  The scans need 64 MiB tables for that (tests/embed_steady_cases.py); the
gather does not, because the CALLER chooses the list order: a table of G tiles runs G workgroups (embed_grid, gather_grid),
workgroup b takes list tiles b, b + G, b + 2G, ... (its ROUNDS), so `steady_list` hands workgroup b any rows in any order
out of a table of 4096 rows.

The gather states the scan's list rules (trigger, capacity, tile size, the final compaction) in its own words; constants()
finds each as text in embed_cand.hip.h, and the two grid rules in embed_cand_request.h and embed_device.hip.h, so Layout,
occupancy and min_rounds of tests/embed_steady_cases.py are the gather's model too and cannot drift from it unnoticed.
`landing` is the gather's finite_counts: the keys a workgroup can append per round, from the list alone.  The reference of
every answer stays tests/embed_oracle.py over the listed rows."""
import functools
import re

import numpy as np

from tests import embed_oracle as eo
from tests import embed_steady_cases as sc

F32 = np.float32
STORAGES = ["f32", "fp16", "bf16"]
DIMS = sc.DIMS
ROWS = 4096          # every table: G tiles of t rows, G = ROWS / t <= MAX_GRID
MAX_GRID = 64
PLATEAU_TOPNS = [10, 128, 1024]


# ---- constants and rules, from the sources ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def constants():
    """sc.constants(), after every rule the model mirrors has been found in the gather's own sources as text."""
    k = sc.constants()
    cand = (sc.CSRC / "embed_cand.hip.h").read_text()
    req = (sc.CSRC / "embed_cand_request.h").read_text()
    dev = (sc.CSRC / "embed_device.hip.h").read_text()
    # the trigger: c >= min(max(2 * topk, floor), kCandLimit), the scan's floor
    m = re.search(r"int compact_at = 2 \* a\.topk > (\d+) \? 2 \* a\.topk : \1;\s*if \(compact_at > kCandLimit\) compact_at = kCandLimit;", cand)
    assert m and int(m.group(1)) == k["compact_floor"]
    assert re.search(r"if \(c >= compact_at\)", cand)
    # ... which calls the scan's compaction (the kept range [topk, topk + slack] is core.hip.h's) and keeps the larger threshold
    assert cand.count("compact_candidates<kEmbedBlock, kCandPerThread>(s_cand, &s_count, a.topk, false, s_sel)") == 2
    assert "if (local_thr > thr) thr = local_thr;" in cand
    # the tile and the capacities
    assert "constexpr int kGroup = kDimT / Rows::kVals;" in cand
    assert "constexpr int kTileEntries = kEmbedTileVecs / kGroup;" in cand
    assert "constexpr int kMaxTileRows = kEmbedTileVecs / (16 / Rows::kVals);" in cand
    assert "constexpr int kCandCap = kCandLimit + kMaxTileRows;" in cand
    assert "__shared__ uint64_t s_cand[kCandCap];" in cand
    assert k["kEmbedTileVecs"] == k["kEmbedBlock"] * k["kEmbedVecsPerThread"]
    # the final compaction and the ranking
    assert re.search(r"if \(s_count > kRankCountMax && s_count > a\.topk\)", cand)
    # the rounds of a workgroup
    assert "int64_t tile = blockIdx.x;" in cand and "for (; tile < n_tiles; tile += gridDim.x) {" in cand
    assert "const int64_t n_tiles = (m + kTileEntries - 1) / kTileEntries;" in cand
    # the two grid rules: min(list tiles, min(table tiles, 2 * CUs, kMergeMaxLists))
    assert re.search(r"inline int gather_grid\(int64_t m, int tile_entries, int scan_grid\) \{\s*"
                     r"const int64_t tiles = \(m \+ tile_entries - 1\) / tile_entries;\s*"
                     r"return static_cast<int>\(tiles < scan_grid \? tiles : scan_grid\);\s*\}", req)
    assert re.search(r"int embed_grid\(int64_t n, int dim, int vals, int cus\) \{\s*"
                     r"const int64_t n_tiles = \(n \* \(dim / vals\) \+ kEmbedTileVecs - 1\) / kEmbedTileVecs;\s*"
                     r"const int64_t grid = std::min<int64_t>\(std::min<int64_t>\(n_tiles, 2 \* cus\), kMergeMaxLists\);\s*"
                     r"return static_cast<int>\(std::max<int64_t>\(grid, 1\)\);\s*\}", dev)
    return k


def layout_of(storage, d):
    """sc.Layout of a gather: tile_rows is kTileEntries, capacity is kCandCap."""
    return sc.Layout(storage, d, constants())


def table_grid(n, t, compute_units):
    """embed_grid of a table of n rows whose tile holds t of them."""
    return max(min(-(-n // t), 2 * int(compute_units), constants()["kMergeMaxLists"]), 1)


def gather_grid(m, t, scan_grid):
    return min(-(-m // t), scan_grid)


def rounds_until(layout, topn, appends=(), compactions=2):
    """`appends`, then as many full tiles as it takes for the model to have compacted `compactions` times in the loop."""
    out = [int(x) for x in appends]
    while sc.occupancy(layout, out, topn)["compactions"] < compactions:
        out.append(layout.tile_rows)
    return out


# ---- the list -----------------------------------------------------------------------------------------------------------

def hostile(n, row_base=0):
    """The ids of tests/test_gpu_embed_cand._lists that name no row of the table."""
    from tests.test_gpu_embed_cand import _lists
    return _lists(n, 8, np.random.default_rng(0), row_base)["outside"]


def free_slots(t, G, b, rounds):
    """The entries of steady_list that are not workgroup b's rounds: (rounds * G + b) full tiles less b's, and the tail."""
    return (rounds * G + b - rounds) * t + t // 2 + 1


def steady_list(n, t, G, b, rounds_rows, filler):
    """LOCAL ids (add row_base for the call).  len(rounds_rows) * G + b full tiles and a partial last tile of t // 2 + 1
    entries, whose index is = b modulo G: it is workgroup b's too, one round behind its last.  Tile r * G + b holds
    rounds_rows[r] (at most t local rows, padded with -1); every other entry, the tail last, takes `filler` in order
    (free_slots() ids: the table's other rows and ids outside it)."""
    R = len(rounds_rows)
    filler = np.asarray(filler, np.int64)
    assert 0 <= b < G and filler.size == free_slots(t, G, b, R)
    tiles = np.full((R * G + b + 1, t), -1, np.int64)
    mine = np.zeros(tiles.shape[0], bool)
    for r, rows in enumerate(rounds_rows):
        rows = np.asarray(rows, np.int64)
        assert rows.size <= t and (rows.size == 0 or (rows.min() >= 0 and rows.max() < n))
        tiles[r * G + b, : rows.size] = rows
        mine[r * G + b] = True
    ids = tiles.reshape(-1)[: (R * G + b) * t + t // 2 + 1]
    free = np.repeat(~mine, t)[: ids.size]
    ids[free] = filler
    return ids.copy()


def filler_of(n, rounds_rows, t, G, b, rng, row_base=0, twice=False):
    """Every row of the table that is in no round, once, and ids outside the table, shuffled; `twice`: every row of the
    rounds a second time among them (in tiles of other workgroups).  The tail (workgroup b's) holds ids outside the table."""
    used = np.concatenate([np.asarray(r, np.int64) for r in rounds_rows])
    rest = np.setdiff1d(np.arange(n, dtype=np.int64), used)
    slots = free_slots(t, G, b, len(rounds_rows))
    tail = t // 2 + 1
    body = np.concatenate([rest, used]) if twice else rest
    assert body.size <= slots - tail
    out = np.concatenate([body, np.resize(hostile(n, row_base) - row_base, slots - tail - body.size)])
    rng.shuffle(out)
    return np.concatenate([out, np.resize(hostile(n, row_base) - row_base, tail)])


def landing(ids, v, n, row_base, t, G):
    """[G, rounds]: the distinct rows with a finite v that workgroup b meets in round r — the keys it can append there.
    Of a row listed more than once the FIRST entry counts (on the GPU any one copy does: the TWICE case)."""
    ids = np.asarray(ids, np.int64)
    inside = (ids >= 0) & (ids >= row_base) & (ids < row_base + n)
    local = np.where(inside, ids - row_base, 0)
    first = np.zeros(ids.size, bool)
    first[np.unique(np.where(inside, local, n), return_index=True)[1]] = True
    ok = inside & first & np.isfinite(np.asarray(v, F32))[local]
    tiles = -(-ids.size // t)
    rounds = -(-tiles // G)
    full = np.zeros(rounds * G * t, bool)
    full[: ids.size] = ok
    return full.reshape(rounds, G, t).sum(axis=2).T


def claimed_rows(ids, n, row_base):
    """The sorted distinct local rows a list names: what the claim keeps."""
    ids = np.asarray(ids, np.int64)
    inside = (ids >= 0) & (ids >= row_base) & (ids < row_base + n)
    return np.unique(ids[inside] - row_base)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _cases():
    out = []
    for storage in STORAGES:
        for d in DIMS:
            for what in ["cosine", "dot"] + (["audio"] if d in (32, 128) else []):
                out.append(("rising", storage, d, what))      # (and FALLING: the same list, every weight negated)
    for storage in STORAGES:
        for d in DIMS:
            out += [("fullest", storage, d, "-1"), ("fullest", storage, d, "nan")]
    out += [("plateau", storage, d, "cosine") for storage in STORAGES for d in DIMS]
    out += [("twice", storage, d, "dot") for storage in STORAGES for d in DIMS]
    return out


CASES = _cases()
RISING = [c for c in CASES if c[0] == "rising"]
FULLEST = [c for c in CASES if c[0] == "fullest"]
PLATEAU = [c for c in CASES if c[0] == "plateau"]
TWICE = [c for c in CASES if c[0] == "twice"]
BASED = ("rising", "f32", 32, "audio")   # the rising case that is also built over row_base = 1 000 000


def case_id(case):
    return "-".join(str(x) for x in case)


class Built:
    """One case: the table (float32, already widened from its storage: converting it again is exact), the request, the
    oracle's v of every row, the list (global ids) and what the model is to say of workgroup b."""


def _store(table, storage):
    if storage == "f32":
        return table
    from spotify_recommender_amd.embed_half import to_storage, widen
    return widen(to_storage(table, storage), storage)


def _values(wide, feats, req):
    return eo.values(wide, req["user"], eo.DOT if req["metric"] == "dot" else eo.COSINE, req["embed_weight"], req.get("audio_weight", 0.0),
                     feats, req.get("audio"))[0]


def negated(req):
    out = dict(req, embed_weight=-req["embed_weight"])
    if "audio_weight" in req:
        out["audio_weight"] = -req["audio_weight"]
    return out


@functools.lru_cache(maxsize=2)
def build(case, row_base=0):
    family, storage, d, what = case
    index = CASES.index(case)
    o = Built()
    o.case, o.storage, o.d, o.row_base = case, storage, d, row_base
    o.layout = layout = layout_of(storage, d)
    o.t = t = layout.tile_rows
    o.G = G = ROWS // t
    o.n = n = G * t
    o.b = b = index % G
    assert G <= MAX_GRID and n == ROWS
    L = layout.k["kCandLimit"]
    rng = np.random.default_rng(1000 * index + d)
    feats = rng.random((n, 12), dtype=F32)
    wide = _store(rng.standard_normal((n, d), dtype=F32), storage)
    user = rng.standard_normal(d, dtype=F32)
    nan_row = None

    if family == "plateau":
        flat = np.zeros(n, bool)
        flat[rng.choice(n, int(0.4 * n), replace=False)] = True
        wide[flat] = wide[np.argmax(flat)]
        user = wide[np.argmax(flat)].copy()
        req = dict(user=user, metric="cosine", embed_weight=1.0, topn=1024)
        v = _values(wide, feats, req)
        assert np.all(v[flat] == v.max()) and np.all(v[~flat] < v.max())
        others = np.nonzero(~flat)[0]
        others = others[np.argsort(v[others], kind="stable")]
        prefix = others[others.size - L:].reshape(L // t, t)                  # rising rows up to the first compaction at top-1024,
        falling = np.nonzero(flat)[0][::-1]                                   # then the plateau: every later row the better key
        rounds_rows = list(prefix) + np.array_split(falling, max(4, -(-falling.size // t)))
        o.plateau = np.nonzero(flat)[0]
        o.topns = PLATEAU_TOPNS
    else:
        if family == "fullest":
            req = dict(user=user, metric="dot", embed_weight=1.0, topn=1024)
            if what == "nan":
                wide[7] = np.nan
        else:
            req = dict(sc.SINGLE_REQUESTS["dot" if family == "twice" else what], user=user)
            if what == "audio":
                req["audio"] = rng.random(12, dtype=F32)
        # the table is sorted by the request's v (a NaN row goes last), so "the best rows" are the last and a round is a run of ids
        wide, v, feats = sc.rising(wide, _values(wide, feats, req), feats)
        finite = int(np.isfinite(v).sum())
        if family == "fullest":
            # workgroup b enters a tile with kCandLimit - 1 keys (no trigger) and appends a full tile on top
            per_round = rounds_until(layout, 1024, [t] * (L // t - 1) + [t - 1, t])
            nan_row = n - 1 if what == "nan" else None
            assert finite == n - (what == "nan")
        else:
            per_round = [t] * sc.min_rounds(layout, req["topn"])
        bounds = finite - sum(per_round) + np.concatenate([[0], np.cumsum(per_round)])
        assert bounds[0] >= 0
        rounds_rows = [np.arange(bounds[r], bounds[r + 1], dtype=np.int64) for r in range(len(per_round))]
        if nan_row is not None:   # the short entry is a row of the table that forms no key under dot
            short = per_round.index(t - 1)
            rounds_rows[short] = np.concatenate([rounds_rows[short], [nan_row]])
        o.topns = [req["topn"]]
    o.feats, o.wide, o.req, o.nan_row = feats, wide, req, nan_row
    o.v = _values(wide, feats, req)
    o.v.setflags(write=False)
    o.rounds_rows = rounds_rows
    o.rounds = len(rounds_rows)
    filler = filler_of(n, rounds_rows, t, G, b, rng, row_base, twice=family == "twice")
    o.ids = steady_list(n, t, G, b, rounds_rows, filler) + row_base
    alone = np.resize(hostile(n, row_base) - row_base, filler.size)   # the same list with no row of another workgroup's in it
    o.ids_alone = steady_list(n, t, G, b, rounds_rows, alone) + row_base
    o.ids.setflags(write=False)
    o.ids_alone.setflags(write=False)
    # what workgroup b is to meet: its rounds' finite rows, then nothing in the tail (ids outside the table)
    o.intended = [int(np.isfinite(o.v[np.asarray(r, np.int64)]).sum()) for r in rounds_rows] + [0]
    return o


def model(o, ids=None, topn=None):
    """The occupancy model on workgroup b's landing of the built list (or of `ids`)."""
    land = landing(o.ids if ids is None else ids, o.v, o.n, o.row_base, o.t, o.G)
    return sc.occupancy(o.layout, land[o.b], topn or o.topns[-1])


def list_shape(o, ids=None):
    """(tiles of the list, the gather's grid when the table's is G)."""
    m = (o.ids if ids is None else ids).size
    return -(-m // o.t), gather_grid(m, o.t, o.G)


def exclusions(o, req, ids, topn=None):
    """Exactly 1024 global ids: every third of the best 3 * topn listed rows under `req`, ids outside the table, -1 and
    repeats.  And the oracle's v under `req`."""
    v = _values(o.wide, o.feats, req)
    rows = claimed_rows(ids, o.n, o.row_base)
    only = np.full(o.n, np.nan, F32)
    only[rows] = v[rows]
    best, _ = eo.topn(only, 3 * (topn or req["topn"]), (), o.row_base)
    third = best[::3]
    pad = np.concatenate([hostile(o.n, o.row_base), [-1, -1], third[:5]])
    out = np.concatenate([third, np.resize(pad, 1024 - third.size)]).astype(np.int64)
    assert out.size == 1024
    return [int(x) for x in out], v
