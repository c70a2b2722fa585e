"""The cases of the parity sweep of the matrix-core batch path (tests/test_gpu_batched_sweep.py on the MI355X,
tests/test_batched_sweep_cpu.py through the CPU backend): row counts around every boundary the host code and the kernels
branch on, batch sizes at the edges of the NB ladder, topn at kMultiMaxTopK, hostile catalogues, shards with a row_base,
duplicate queries, the served / queued edge of the pre-filter, step 2 of pass 1 and the exact multi-query pass across its chain.

The bar is the project's usual one: score bits equal to oracle.scores, ids tie-aware against oracle.topn_heap
(tests.parity.assert_topn_matches), the count, and -1 / +0.0 past it.

Where every number below comes from (csrc/ = spotify_recommender_amd/csrc/):

  rows
    1, 2               one row / two rows: every group of pass 1 but one is empty, `row < n ? row : last_row` clamps every
                       lane of the only tile (batched.hip.h:390-406)
    31, 32, 33         32 rows = one MFMA sub-tile (A[0] of batched.hip.h:550-552); 33 puts one row into the second
    63, 64, 65         n_tiles = (n + 63) / 64 (engine_batch.hip.h:491): one full wave tile, and one row into the second
    127, 128, 129      kMultiMaxTopK = 128 (kernels.hip.h:353): the sync call's eff = min(topn, n) (mi355rec.hip:903) reaches
                       128 only from 128 rows on, and topn = 129 leaves the path only from 129 rows on
    1023, 1024, 1025   kBqNbhdRows = 1024 (batched.hip.h:86): a neighbourhood of bq_prepare_kernel is 1024 rows; also the
                       tile of the exact queue's scan (MultiConfig::kTileRows: qgrid = min(cus, tiles), engine_batch.hip.h:399-402)
    2047, 2048, 2049   kNbhdRows = 2048 (handoff.hip.h:44): `nbhd = h->n >= kNbhdRows` (engine_batch.hip.h:502) — from here
                       on bq_prepare_kernel carries a neighbourhood workgroup per query and the handle has an anchor table
    4095, 4096, 4097   kAnchorRows = 4096 (handoff.hip.h:310): anchor i is row i below it, a strided sample from it on
    8193               129 wave tiles: 8 exact-queue tiles, and more tiles than one pass workgroup's four waves see in 32
                       rounds; like every count up to here, fewer tiles than the pass grid has waves (b.grid up to 1280
                       workgroups of 4 waves, batched.hip.h:384-385), so most workgroups of both passes find no tile at all
    65 535 / 6 / 7     kBqMinRows = kReplicaMinRows = 65 536 (engine_batch.hip.h:352): from here the handle has an fp16
                       replica, launch_bq_passes takes the replica-sourced kernels (:544) and tile_max is allocated (:438-447)
    131 073            cand_cap doubles while cand_cap * 64 < n (engine_batch.hip.h:411-412): 2048 up to 131 072 rows, 4096 past it

  batch sizes          nb = next power of two of ceil(count / 32) (engine_batch.hip.h:564-566): 32 -> NB 1; 33, 64 -> 2;
                       65, 128 -> 4; 129, 256 -> 8; 257, 512 -> 16; 513, 1024 -> 32; 1025 = a chunk of 1024 and a chunk of
                       ONE query (engine_batch.hip.h:622-623).  NB >= 16 with a replica is the kTileMax form (:546-549).

  the served / queued edge — see pass1_groups() and claimable_served() below.

  step 2               bq_step1 (engine_batch.hip.h:366-371) — see step2_rows() below.

  chain                kMultiChain = 36 (kernels.hip.h:352): enqueue_batch cuts a BATCH_MULTI batch into chains of 36
                       (engine_batch.hip.h:657-658), a chain into passes of kMultiQueries = 12.
"""
import ctypes
import functools

import numpy as np

from oracle import oracle
from tests.parity import assert_topn_matches
from tests.test_gpu_fuzz import make_catalogue

SEED = 20261018

# capi's constants, repeated so that this module imports without the library
BATCH_AUTO, BATCH_MULTI, BATCH_MFMA, BATCH_MFMA_NOSKIP = 0, 1, 2, 5
REPLICA_AUTO, REPLICA_OFF, REPLICA_ON = 0, 1, 2

K_MULTI_MAX_TOPK = 128      # kernels.hip.h:353
K_BQ_MAX_QUERIES = 1024     # batched.hip.h:74
K_BQ_SPECIAL_CAP = 1024     # batched.hip.h:85
K_NBHD_ROWS = 2048          # handoff.hip.h:44
K_BQ_MIN_ROWS = 65_536      # engine_batch.hip.h:352
K_BQ_MIN_NORM2, K_BQ_MAX_NORM2 = 1.01e-8, 1e36   # batched.hip.h:101-102

UNIFORM = "u"               # oracle.mt19937_uniform; 0 .. 6 are make_catalogue's kinds
KIND_NAMES = {UNIFORM: "mt19937 uniform", 0: "uniform", 1: "mass ties", 2: "clusters", 3: "signed wide", 4: "sorted", 5: "duplicates",
              6: "sparse special"}

ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193,
        65_535, 65_536, 65_537, 131_073)
STARRED = (32, 64, 65, 2048, 4096, 65_535, 65_536, 65_537)      # also with 32 and 513 queries
ROW_CLASSES = {                                                   # a test id per class
    "le129": (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129),
    "1024": (1023, 1024, 1025),
    "2048": (2047, 2048, 2049),
    "4096": (4095, 4096, 4097, 8193),
    "65535": (65_535,), "65536": (65_536,), "65537": (65_537,), "131073": (131_073,),
}
assert sorted(n for c in ROW_CLASSES.values() for n in c) == sorted(ROWS)
BATCHES = (32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
BATCH_ROWS = (4097, 65_537)
TOPNS = (1, 10, 127, 128, 129)
HOSTILE_KINDS = (1, 2, 3, 4, 5, 6)
HOSTILE_ROWS = (300, 2049, 7000, 40_000)
HOSTILE_BATCHES = (40, 130)
SOURCE_ROWS = (65_537, 131_073)
CHAIN_BATCHES = (35, 36, 37, 72, 73)
CHAIN_ROWS = (65, 2049, 40_000)
CHAIN_TOPNS = (1, 128)
CPU_MAX_ROWS, CPU_MAX_BATCH = 4097, 129


def nb_of(count: int) -> int:
    """enqueue_bq_chunk's NB of a chunk of `count` queries (engine_batch.hip.h:564-566)."""
    blocks, nb = (count + 31) // 32, 1
    while nb < blocks:
        nb *= 2
    return nb


assert [nb_of(b) for b in BATCHES[:-1]] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32] and nb_of(1025 - 1024) == 1


# ---- the served / queued edge -------------------------------------------------------------------------------------------
# Pass 1 (bq_pass_kernel<NB, false>, batched.hip.h:384-385): wave w of workgroup g starts at tile (4 g + w) * tile_step and
# moves on by grid * 4 * tile_step; tile_step = 1 below grid * 64 tiles (bq_step1).  So while a shard has no more tiles than
# the grid has waves, tile t is looked at by wave t % 4 of workgroup t / 4, once.
# A lane of the wave holds, of each 32-row sub-tile, the rows (i & 3) + 8 (i >> 2) + 4 h, h = lane >> 5 (the C/D layout,
# batched.hip.h:231-232): the rows whose bit 2 is h.  The group maxima are kept per (workgroup, lane half): group =
# half * grid + workgroup (batched.hip.h:800).  So half 0 of a tile is non-empty from its first row on, half 1 from its fifth.
# bq_select_kernel (batched.hip.h:861-870) claims a threshold from the groups only when topn + 1 of them have a maximum > 0;
# against a catalogue of positive rows every non-empty group has one.
def pass1_groups(n: int) -> int:
    """Non-empty (workgroup, lane half) groups of pass 1 over n rows (n small enough for one tile per wave)."""
    tiles = (n + 63) // 64
    assert tiles <= 4 * 256, "derived for shards with no more tiles than a grid of 256 workgroups has waves"
    groups = 2 * ((tiles + 3) // 4)
    if tiles % 4 == 1 and n - (tiles - 1) * 64 <= 4:    # the last workgroup has ONE tile, with rows in half 0 only
        groups -= 1
    return groups


def groups_edge(topn: int) -> int:
    """The smallest row count with topn + 1 non-empty groups."""
    n = 1
    while pass1_groups(n) < topn + 1:
        n += 1
    return n


# topn + 1 = 2 groups: rows 0 .. 3 and row 4 of tile 0                                    -> 5 rows
# 11 groups: workgroups 0 .. 4 (tiles 0 .. 19) give ten, the first row of tile 20 the 11th  -> 20 * 64 + 1 = 1281 rows
# 129 groups: workgroups 0 .. 63 (tiles 0 .. 255), the first row of tile 256                -> 256 * 64 + 1 = 16 385 rows
assert [groups_edge(t) for t in (1, 10, 128)] == [5, 1281, 16_385]

# The groups are not the only source of a threshold.  From kNbhdRows = 2048 rows on (engine_batch.hip.h:502) bq_prepare_kernel
# computes every query's NEIGHBOURHOOD bound (the exact topn-th best of up to 1024 rows around its excluded row, or around its
# anchor: batched.hip.h:175-193) and bq_select_kernel takes the larger of the two (batched.hip.h:871-876).  A shard of fewer
# than 2048 rows has at most 32 tiles = 8 workgroups = 16 groups, so:
#   topn <= 15: the edge is the groups' (5 rows for top-1, 1281 for top-10), below kNbhdRows, where nothing else helps;
#   topn >= 16: no row count below 2048 serves a query and every row count from 2048 on does — through the neighbourhood.
#               For top-128 the edge is kNbhdRows itself, NOT the 16 385 rows of the groups: at 16 321 rows (one tile
#               below) every claimable query is served.  (The sweep found this by its counters; the kernel is right, a
#               derivation from the groups alone is not.)
# The host switches the neighbourhood workgroups off on a handle after kBqNbProbeChunks = 3 chunks in which no bound beat
# the groups' (engine_batch.hip.h:503-508), so a case that depends on them is the FIRST batched call on its handle.
EDGE_CASES = (
    # (topn, rows, every claimable query served?)
    (1, 4, False), (1, 5, True), (1, 5 + 64, True),                       # (one tile below 5 rows is no shard: one ROW below)
    (10, 1281 - 64, False), (10, 1281, True), (10, 1281 + 64, True),
    (128, 2048 - 64, False), (128, 2047, False), (128, 2048, True), (128, 2048 + 64, True),
    (128, 16_385 - 64, True), (128, 16_385, True), (128, 16_385 + 64, True),
)


def claimable_served(n: int, eff: int) -> bool:
    """Is a query the bound can be claimed for served by the pre-filter — uniform positive rows, the first batched call on
    a handle?  eff = min(topn, n)."""
    if n >= K_NBHD_ROWS:
        return True
    return pass1_groups(n) >= eff + 1


for _t, _n, _s in EDGE_CASES:
    assert claimable_served(_n, min(_t, _n)) == _s, (_t, _n)


# ---- step 2 of pass 1 -------------------------------------------------------------------------------------------------
# bq_step1 (engine_batch.hip.h:366-371): step1 = 1 below grid * (kBqPassBlock / 64 = 4) * 16 tiles; from there b.step1 = 4
# halved while n_tiles < grid * 4 * 8 * step1: 2 from grid * 64 tiles on, 4 from grid * 128.  grid = b.grid = CUs x
# occupancy, at most kBqMaxPassGrid = 1280 (engine_batch.hip.h:390-392), reported as stats().batched_grid_blocks.
def step2_rows(grid: int):
    """(the smallest row count with step1 == 2, one tile more with a ragged last tile) — 5 242 880 and 5 242 941 at 1280."""
    tiles = grid * 4 * 16
    return tiles * 64, tiles * 64 + 64 - 3


def step1_of(n: int, grid: int) -> int:
    n_tiles = (n + 63) // 64
    step = 4 if n_tiles >= grid * 4 * 16 else 1
    while step > 1 and n_tiles < grid * 4 * 8 * step:
        step //= 2
    return step


assert step2_rows(1280) == (5_242_880, 5_242_941)
assert step1_of(5_242_880, 1280) == 2 and step1_of(5_242_879 - 63, 1280) == 1 and step1_of(5_242_941, 1280) == 2


# ---- catalogues and queries -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def catalogue(n: int, kind):
    """mt19937 uniform rows (kind UNIFORM) or make_catalogue's kind 0 .. 6 (tests/test_gpu_fuzz.py: reused, not copied)."""
    if kind == UNIFORM:
        f = oracle.mt19937_uniform(SEED % 100_000 + n, n)
    else:
        f = make_catalogue(np.random.default_rng([SEED, kind, n]), n, kind=kind)
    f = np.ascontiguousarray(f, dtype=np.float32)
    f.setflags(write=False)
    return f


def uniform_kind_at(n: int):
    """The uniform catalogues alternate between the two generators."""
    return UNIFORM if n not in ROWS or ROWS.index(n) % 2 == 0 else 0


class Case:
    """One batched call.  `excl` holds GLOBAL ids (row_base + local row), -1 = none."""

    def __init__(self, what, n, kind, batch, topn, row_base=0, path=BATCH_MFMA, replica=REPLICA_AUTO, variant=""):
        self.what, self.n, self.kind, self.batch, self.topn = what, int(n), kind, int(batch), int(topn)
        self.row_base, self.path, self.replica, self.variant = int(row_base), path, replica, variant
        self.eff = min(self.topn, self.n)
        self.uniform = kind in (UNIFORM, 0)

    def __repr__(self):
        return (f"{self.what}: n={self.n} [{KIND_NAMES[self.kind]}] batch={self.batch} top-{self.topn}"
                + (f" row_base={self.row_base}" if self.row_base else "") + (f" {self.variant}" if self.variant else ""))

    @property
    def on_path(self) -> bool:
        """use_bq (engine_batch.hip.h:610-616) with the path forced."""
        return self.path in (BATCH_MFMA, BATCH_MFMA_NOSKIP) and self.eff <= K_MULTI_MAX_TOPK

    @property
    def chunks(self) -> int:
        return (self.batch + K_BQ_MAX_QUERIES - 1) // K_BQ_MAX_QUERIES

    def feats(self):
        return catalogue(self.n, self.kind)

    def queries(self):
        """(queries [batch, 12], excluded global ids [batch], the slots of the unclaimable queries)."""
        return _build_queries(self.n, self.kind, self.batch, self.row_base, self.variant, self.uniform)

    def local_exclude(self, e: int) -> int:
        e -= self.row_base
        return int(e) if 0 <= e < self.n else -1

    def expected_count(self, e: int) -> int:
        return min(self.topn, self.n - (1 if self.local_exclude(e) >= 0 else 0))


def unclaimable_slots(batch: int):
    """Where the zero, tiny, huge and NaN queries sit (none in a batch of fewer than 8): never the last slot, so that the
    one-query chunk of a 1025-query batch is a query the pre-filter serves."""
    return (2, batch // 2, batch - 5, batch - 2) if batch >= 8 else ()


@functools.lru_cache(maxsize=8)
def _build_queries(n, kind_key, batch, row_base, variant, uniform):
    feats = catalogue(n, kind_key)
    rng = np.random.default_rng([SEED, n, batch, row_base % 1000, len(variant)])
    q = np.empty((batch, 12), np.float32)
    e = np.full(batch, -1, np.int64)
    perm = rng.permutation(n)
    perm = np.concatenate([perm[perm != n - 1], [n - 1]])                                    # (the last row is taken on purpose, below)
    own, by_value = list(perm[: (batch + 3) // 4]), list(perm[::-1][1: 1 + (batch + 3) // 4])   # (disjoint once n > batch / 2)
    clean = lambda r: np.nan_to_num(feats[int(r)], nan=0.5, posinf=1.0, neginf=-1.0).astype(np.float32)
    for b in range(batch):
        t = b % 4
        if t == 0 and own:                      # a row of the catalogue, its own id excluded (recommendByIndex)
            r = int(own.pop())
            q[b], e[b] = feats[r], row_base + r
        elif t == 1 and by_value:               # a row passed by value, nothing excluded: it is its own best match
            # (the first of them is the LAST row: a pass that drops the partial last tile loses this list's best row)
            r = n - 1 if b == 1 else int(by_value.pop())
            q[b] = feats[r]
        elif t <= 2:                            # a perturbed row; every other one excludes an arbitrary row
            q[b] = clean(rng.integers(0, n)) * np.float32(1.01) + np.float32(0.01) * rng.random(12, dtype=np.float32)
            if b % 8 >= 4:
                e[b] = row_base + int(rng.integers(0, n))
        else:                                   # noise
            q[b] = rng.random(12, dtype=np.float32)
    bad = unclaimable_slots(batch)
    if bad:
        noise = rng.random((4, 12), dtype=np.float32) + np.float32(0.05)
        q[bad[0]] = 0.0                                   # zero
        q[bad[1]] = noise[1] * np.float32(1e-6)           # |q| < 1.005e-4 (kBqMinNorm)
        q[bad[2]] = noise[2] * np.float32(1e19)           # |q| > 1e18 (kBqMaxNorm)
        q[bad[3]] = noise[3]
        q[bad[3], 4] = np.nan
        assert float(np.linalg.norm(q[bad[1]].astype(np.float64))) < 1.005e-4 and float(np.linalg.norm(q[bad[2]].astype(np.float64))) > 1e18
        for s in bad:
            e[s] = -1
    if variant == "shard":
        # excluded ids that lie in ANOTHER shard (below row_base, and past the end), and the LAST row of this one (in a
        # partial tile at 65 and 4097 rows), asked for by that row itself
        free = [b for b in range(batch) if b not in bad]
        e[free[1]] = max(row_base - 1, 0) if row_base else n + 7        # the row below this shard
        e[free[2]] = free[2] % n                                        # a local index without the base: shard 0's row
        e[free[3]] = row_base + n                                       # the first row of the next shard
        e[free[5]] = 4_000_000_000                                      # far past every shard
        q[free[0]], e[free[0]] = feats[n - 1], row_base + n - 1
        q[free[4]], e[free[4]] = q[free[7]], row_base + n - 1           # another query excludes the last row
    if variant == "duplicates":
        # the same query twice in one batch, with different excluded rows: its own, and another query's
        free = [b for b in range(0, batch - 4, 4) if e[b] >= 0 and not {b, b + 1, b + 3} & set(bad)]
        a, b2, c = free[0], free[1], free[2]
        for dst in (a + 1, batch - 1):
            assert dst not in bad
            q[dst] = q[a]
        e[a + 1] = e[b2]
        e[batch - 1] = -1
        q[c + 3] = q[c]                                                 # a noise slot: same vector, the SAME exclusion
        e[c + 3] = e[c]
    if uniform and variant != "duplicates":
        keyed = {(q[b].tobytes(), int(e[b])) for b in range(batch)}
        assert len(keyed) == batch, "the queries of a case are pairwise distinct"
    q.setflags(write=False)
    e.setflags(write=False)
    return q, e, tuple(bad)


def special_rows(feats) -> int:
    """Rows that are neither valid (|row|^2 in [kBqMinNorm2, kBqMaxNorm2]) nor exactly zero (batched.hip.h:526-530), in the
    kernel's fp32: a square that underflows is zero, one that overflows is inf."""
    with np.errstate(all="ignore"):
        tot = (feats.astype(np.float32) ** 2).astype(np.float64).sum(axis=1)
        tot32 = tot.astype(np.float32)
    valid = (tot32 >= np.float32(K_BQ_MIN_NORM2)) & (tot32 <= np.float32(K_BQ_MAX_NORM2))
    return int(np.count_nonzero(~valid & ~(tot32 == 0)))


def expected_counters(case: Case):
    """What mi355rec_batched_last_counters must report for the LAST chunk of the call — a uniform catalogue, the first
    batched call on the handle where the neighbourhood matters: {"queued_queries", "served"}; None where nothing is claimed
    (kinds 1 to 6: results right, no more)."""
    if not case.on_path or not case.uniform:
        return None
    first = (case.batch - 1) // K_BQ_MAX_QUERIES * K_BQ_MAX_QUERIES
    real = case.batch - first
    bad = sum(1 for s in unclaimable_slots(case.batch) if s >= first)
    if claimable_served(case.n, case.eff):
        return {"queued_queries": bad, "served": real - bad}
    return {"queued_queries": real, "served": 0}


def check_counters(case: Case, d: dict):
    want = expected_counters(case)
    if want is not None:
        assert d["queued_queries"] == want["queued_queries"], f"{case}: {d}, expected {want}"
        assert d["candidates_total"] >= want["served"], f"{case}: {d}, expected {want}"
        if want["served"] == 0:
            assert d["candidates_total"] == 0, f"{case}: {d}"
    if case.on_path:
        sp = special_rows(case.feats())
        if sp <= K_BQ_SPECIAL_CAP:
            assert d["special_rows"] == sp, f"{case}: {d}, {sp} special rows in the catalogue"


# ---- the check of one list ---------------------------------------------------------------------------------------------
def check_query(case: Case, b: int, got_idx, got_score, queries, excl):
    """Query b's list (GLOBAL ids, cut to its count) against the oracle: tests.parity.assert_topn_matches with
    oracle.topn_heap.  On a large shard both run over the rows that can matter — every row at or above the topn-th best
    score (all of a boundary tie) and the excluded row; a returned row outside them fails first — instead of sorting
    65 537 scores a thousand times."""
    feats, n, topn = case.feats(), case.n, case.topn
    s = oracle.scores(feats, queries[b])
    ex = case.local_exclude(int(excl[b]))
    idx = np.asarray(got_idx, np.int64) - case.row_base
    try:
        assert len(idx) == case.expected_count(int(excl[b])), f"count {len(idx)}, expected {case.expected_count(int(excl[b]))}"
        if n > 8192 and topn < n // 8:
            m = s.astype(np.float64)
            if ex >= 0:
                m[ex] = -np.inf
            kth = np.partition(m, n - topn)[n - topn]
            keep = np.flatnonzero(m >= kth)
            if ex >= 0:
                keep = np.sort(np.append(keep, ex))
            assert np.all((idx >= 0) & (idx < n)), "a row outside the shard"
            pos = np.searchsorted(keep, idx)
            assert np.all(pos < len(keep)) and np.array_equal(keep[np.minimum(pos, len(keep) - 1)], idx), \
                f"rows below the top-{topn} score: {idx[~np.isin(idx, keep)][:8]}"
            s2 = np.ascontiguousarray(s[keep])
            ex2 = int(np.searchsorted(keep, ex)) if ex >= 0 else -1
            assert_topn_matches(pos, got_score, s2, ex2, topn, ref_idx=oracle.topn_heap(s2, ex2, topn))
        else:
            assert_topn_matches(idx, got_score, s, ex, topn, ref_idx=oracle.topn_heap(s, ex, topn))
    except AssertionError as err:
        raise AssertionError(f"{case}: query {b} (excluded {int(excl[b])}): {err}") from err


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def batch_padded(obj, queries, excl, topn):
    """mi355rec_query_batch_topn (a CosineEngine) or mi355rec_sharded_query_batch_topn (a NodeEngine) with the output
    buffers filled with 7s first: asserts every count in [0, topn] and -1 / +0.0 past it; returns (idx, score, counts)."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import CosineEngine
    node = not isinstance(obj, CosineEngine)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 12)
    b = q.shape[0]
    ex = np.ascontiguousarray(excl, dtype=np.int64).reshape(b)
    idx, sc, counts = np.full((b, topn), 7, np.int64), np.full((b, topn), 7, np.float32), np.full(b, -5, np.int32)
    fn = obj._lib.mi355rec_sharded_query_batch_topn if node else obj._lib.mi355rec_query_batch_topn
    rc = fn(obj._h, _ptr(q), b, _ptr(ex), int(topn), _ptr(idx), _ptr(sc), _ptr(counts))
    obj._check(rc) if node else capi.check(rc, obj._h)
    assert np.all((counts >= 0) & (counts <= topn)), counts
    past = np.arange(topn)[None, :] >= counts[:, None]
    assert np.all(idx[past] == -1), f"ids past the count: queries {np.flatnonzero((past & (idx != -1)).any(axis=1))[:8]}"
    assert not sc.view(np.uint32)[past].any(), f"scores past the count: queries {np.flatnonzero((past & (sc.view(np.uint32) != 0)).any(axis=1))[:8]}"
    assert np.all(idx[~past] >= 0), "a row id below 0 inside the count"
    return idx, sc, counts


# ---- the case lists ----------------------------------------------------------------------------------------------------
def row_cases(n: int):
    """Every row count x 33 queries (NB = 2, 31 pads), top-10; the starred ones also x 32 (NB = 1, no pad) and 513 (NB = 32:
    kTileMax from 65 536 rows on); below 129 rows also topn = 129 > n (eff = n: the call stays on the path).  Where the
    neighbourhood decides (2048 rows and more, topn >= 16) that case comes FIRST on the handle."""
    kind = uniform_kind_at(n)
    out = [Case("rows", n, kind, 33, 10)]
    if n in STARRED:
        out += [Case("rows", n, kind, 32, 10), Case("rows", n, kind, 513, 10)]
    if n < 129:
        out.append(Case("topn > n", n, kind, 33, 129))
    return out


def batch_cases(n: int):
    """The NB ladder at 4097 rows (fp32-sourced: no replica below 65 536) and at 65 537 (replica-sourced, kTileMax from 257 on)."""
    return [Case("batch sizes", n, UNIFORM, b, 10) for b in BATCHES]


def topn_cases(n: int):
    """topn 1, 10, 127, 128 on the path, 129 off it (use_bq: topn > kMultiMaxTopK, engine_batch.hip.h:611); top-128 first:
    at 4097 rows its threshold is the neighbourhood's."""
    return [Case("topn", n, UNIFORM, 33, t) for t in (128, 127, 1, 10, 129)]


def hostile_cases(kind: int, n: int):
    """Kinds 1 to 6: mass ties overflow a candidate list and queue the query (batched.hip.h:935), special rows below and
    above kBqSpecialCap, zero rows.  Results right; no counter but special_rows is claimed."""
    topns = (1, 10, 127, 128)
    i = HOSTILE_KINDS.index(kind) + HOSTILE_ROWS.index(n)
    return [Case("hostile", n, kind, 40, topns[i % 4]), Case("hostile", n, kind, 130, topns[(i + 2) % 4])]


def source_cases(n: int):
    """(case, ways): every case at 65 537 / 131 073 rows replica-sourced (the default), fp32-sourced (REPLICA_OFF) with
    identical keys, and — 513 and 1024 queries, NB = 32 — BATCH_MFMA_NOSKIP with keys identical to the kTileMax run
    (engine_batch.hip.h:544-556).  The 1024-query case runs at 65 537 rows only: at 131 073 it was the costliest case of the file."""
    return [Case("sources", n, UNIFORM, b, 10) for b in ((33, 513, 1024) if n == 65_537 else (33, 513))]


def shard_cases(n: int):
    """row_base = 3 n: bq_finalize_kernel compares row_base + row with the excluded id (batched.hip.h:994-996), the
    neighbourhood takes exclude - row_base (batched.hip.h:182)."""
    return [Case("shard", n, UNIFORM, 33, 10, row_base=3 * n, variant="shard"), Case("shard", n, UNIFORM, 33, 10, variant="shard")]


def duplicate_cases():
    return [Case("duplicates", 4097, UNIFORM, 33, 10, variant="duplicates"), Case("duplicates", 65_537, UNIFORM, 65, 10, variant="duplicates")]


def edge_cases(topn: int):
    return [(Case("edge", n, UNIFORM, 33, topn), served) for t, n, served in EDGE_CASES if t == topn]


def chain_cases(n: int):
    """BATCH_MULTI across kMultiChain = 36 (kernels.hip.h:352): 35 / 36 / 37 and 72 / 73 queries, top-1 and top-128."""
    kind = {65: UNIFORM, 2049: 1, 40_000: 6}[n]
    return [Case("chain", n, kind, b, t, path=BATCH_MULTI) for b in CHAIN_BATCHES for t in CHAIN_TOPNS]


def replica_on_demand_cases():
    """set_replica(REPLICA_ON) builds the fp16 replica of a 4097-row shard (mi355rec.hip:648-659): the replica-sourced
    passes — the staged ring of NB <= 8, kTileMax at NB = 32 — over 65 tiles, far fewer than workgroups."""
    return [Case("replica on demand", 4097, UNIFORM, b, 10, replica=REPLICA_ON) for b in (33, 257, 513)]


def entry_cases():
    """One case per NB for mi355rec_enqueue_batch_keys_dev (device-resident queries), at 4097 rows."""
    return [Case("device-resident", 4097, UNIFORM, b, 10) for b in (32, 64, 128, 256, 512, 1024)]


def cpu_cases():
    """The CPU leg: rows up to 4097, batches up to 129, one shard (a node handle has no row_base)."""
    out = []
    for n in ROWS:
        if n <= CPU_MAX_ROWS:
            out += [c for c in row_cases(n) if c.batch <= CPU_MAX_BATCH]
    out += [c for c in batch_cases(4097) if c.batch <= CPU_MAX_BATCH]
    out += topn_cases(4097)
    for kind in HOSTILE_KINDS:
        for n in HOSTILE_ROWS:
            if n <= CPU_MAX_ROWS:
                out += [c for c in hostile_cases(kind, n) if c.batch <= CPU_MAX_BATCH]
    out += [c for n in (65, 4097) for c in shard_cases(n) if c.row_base == 0]
    out += [c for c in duplicate_cases() if c.n <= CPU_MAX_ROWS]
    out += [c for t in (1, 10, 128) for c, _ in edge_cases(t) if c.n <= CPU_MAX_ROWS]
    out += [c for n in CHAIN_ROWS if n <= CPU_MAX_ROWS for c in chain_cases(n) if c.batch <= CPU_MAX_BATCH]
    return out


def served_coverage():
    """{(NB, source)} of the uniform cases whose LAST chunk the pre-filter must serve (asserted from the counters where they
    run): every NB of the ladder for the fp32-sourced passes (4097 rows) and the replica-sourced ones (65 537 rows), NB 16 and
    32 for kTileMax and NB 32 for NOSKIP."""
    got = set()
    for n in BATCH_ROWS:
        for c in batch_cases(n):
            want = expected_counters(c)
            if want and want["served"] > 0:
                nb = nb_of(c.batch - (c.batch - 1) // K_BQ_MAX_QUERIES * K_BQ_MAX_QUERIES)
                got.add((nb, "fp32" if n < K_BQ_MIN_ROWS else "replica"))
                if n >= K_BQ_MIN_ROWS and nb >= 16:
                    got.add((nb, "tilemax"))
    for n in SOURCE_ROWS:
        for c in source_cases(n):
            if expected_counters(c)["served"] > 0:
                got.add((nb_of(c.batch), "fp32"))
                if nb_of(c.batch) >= 16:
                    got.add((nb_of(c.batch), "noskip"))
    return got
