"""The cases of the size- and edge-case sweep of the playlist kernel family (tests/test_gpu_fuzz_playlist.py on the MI355X,
tests/test_playlist_sweep_cpu.py through the CPU backend): catalogue sizes around every boundary the kernels branch on, the
calls made on each handle, chosen label histograms, the diversified grid — and the raw calls that also check the padding.

Everything is compared with the Python oracles (tests/weighted_oracle.py, filter_oracle.py, labels_oracle.py,
diverse_oracle.py): identical ids, bit-equal scores, bit-equal mmr; the returned count, and -1 / 0.0 / 0.0 past it.

What the API itself rules out, so no list below can hold it:
  * an exclusion list has at most MI355REC_MAX_EXCLUDE = 1024 ids (the members of a by-row call come on top), so "every row
    excluded" and "every row but one" exist up to 1024 rows; above, `exclusion_lists` gives the 1024 LAST rows instead (the
    whole tail of the catalogue, the partial quad included);
  * topn and pool are at most 1024: the values n - n_excl - 1, n - n_excl, n - n_excl + 1 that straddle `eff` are taken
    where they lie in [1, 1024];
  * a node handle refuses an excluded id >= n (ERR_INVALID_ARG, "excluded row ... out of the catalogue") where the
    single-device handle lets it match nothing: `exclusion_lists(n, node=True)` leaves those ids out and the suites assert
    the refusal once.
"""
import ctypes
import functools
import itertools

import numpy as np

from tests.diverse_oracle import LAMBDAS, WHERE, rerank
from tests.diverse_oracle import variants as diverse_variants
from tests.filter_oracle import expected_where
from tests.test_gpu_fuzz import make_catalogue
from tests.weighted_oracle import weight_kinds, weighted_scores

SEED = 20261017

# ---- 1. playlist, filter and weights -------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 65_535, 65_536, 65_537)
SIZE_CLASSES = {                     # handles are made once per size, a test function per class
    "le5": (1, 2, 3, 4, 5),
    "64": (63, 64, 65),
    "256": (255, 256, 257),
    "2048": (2047, 2048, 2049),
    "4096": (4095, 4096, 4097, 8193),
    "65536": (65_535, 65_536, 65_537),
}
CPU_MAX_ROWS = 4097                  # the CPU leg: sizes up to here, one kind each
AUTO_SIZES = (65_535, 65_536, 65_537)
BIG = 65_535                         # from here on k <= 3, except for one k = 32 call
KS = (1, 3, 32)
TOPNS = (1, 10, 256, 257, 1024)      # 256 / 257 straddle kPlBoundRows; "eff-1", "eff", "eff+1" are added per exclusion list
MAX_TOPN = 1024
MAX_EXCLUDE = 1024

# make_catalogue's kinds: 0 uniform, 1 mass ties, 2 tight clusters, 3 signed wide range, 4 sorted towards the ones vector,
# 5 duplicates, 6 sparse rows with NaN / +-inf / denormals / 3e19
PLAIN_KINDS = (0, 2, 4)
HOSTILE_KINDS = (1, 3, 5, 6)
KIND_NAMES = ("uniform", "mass ties", "clusters", "signed wide", "sorted", "duplicates", "sparse special")


def kinds_at(n: int):
    """Two kinds per size, one of them hostile; over SIZES every kind is met.  65 537 rows also get the uniform kind (the
    pre-filter's rows_exact check is stated for it)."""
    i = SIZES.index(n) if n in SIZES else n
    kinds = [PLAIN_KINDS[i % 3], HOSTILE_KINDS[i % 4]]
    if n == 65_537 and 0 not in kinds:
        kinds.insert(0, 0)
    return tuple(kinds)


assert {k for n in SIZES for k in kinds_at(n)} == set(range(7))


def catalogue_of_kind(kind: int, n: int, seed: int = SEED):
    """make_catalogue's catalogue of a chosen kind (tests/test_gpu_fuzz.py: reused, not copied)."""
    return make_catalogue(np.random.default_rng([seed, kind, n]), n, kind=kind)


def ramped(feats):
    """A copy whose feature 0 is the ramp i / n: a filter on it can admit nothing, or exactly the last rows."""
    f = feats.copy()
    n = f.shape[0]
    f[:, 0] = (np.arange(n, dtype=np.float64) / n).astype(np.float32)
    return np.ascontiguousarray(f)


def filters(feats_ramped):
    """{name: where}: none, diverse_oracle.WHERE, one that admits nothing, one that admits only rows >= n - 3."""
    n = feats_ramped.shape[0]
    return {"none": None, "WHERE": WHERE, "nothing": {0: (2.0, 3.0)}, "tail3": {0: (float(feats_ramped[max(n - 3, 0), 0]), 1.0)}}


def exclusion_lists(n: int, node: bool = False):
    """{name: ids}: empty; a few with duplicates and ids >= n; every row; every row but one (see the module's docstring)."""
    few = [0, 0, n // 2, n - 1, n - 1] + ([] if node else [n, n + 7, 4_000_000_000])
    out = {"none": None, "few": few}
    if n <= MAX_EXCLUDE:
        out["all"] = list(range(n))
        out["all_but_one"] = [i for i in range(n) if i != n // 3]
    else:
        out["last1024"] = list(range(n - MAX_EXCLUDE, n))
    return out


def _n_excluded(n, rows, excl):
    ids = set(int(r) for r in (rows if rows is not None else []))
    ids |= set(int(e) for e in (excl or []) if 0 <= int(e) < n)
    return len(ids)


def members_of(rng, feats, k: int):
    """(rows for the by-row call: min(k, n) distinct rows; vectors for the by-value call: a catalogue row, a perturbed one, noise)."""
    n = feats.shape[0]
    rows = rng.choice(n, size=min(k, n), replace=False).astype(np.int64)
    vecs = rng.random((k, 12), dtype=np.float32)
    vecs[0] = np.nan_to_num(feats[int(rng.integers(0, n))], nan=0.5, posinf=1.0, neginf=-1.0)
    if k > 1:
        vecs[1] = (vecs[0] * np.float32(1.01)).astype(np.float32) + np.float32(0.01) * vecs[1]
    return rows, np.ascontiguousarray(vecs)


class Call:
    """One playlist call and what it must return."""

    def __init__(self, what, feats, rows, vecs, weights, excl, where, topn, cache, key):
        self.what, self.rows, self.vecs, self.weights, self.excl, self.where, self.topn = what, rows, vecs, weights, excl, where, int(topn)
        members = feats[rows] if rows is not None else vecs
        w = np.ones(len(members), np.float32) if weights is None else np.asarray(weights, np.float32)
        if key not in cache:                                   # the O(n k) part, once per (members, weights)
            cache[key] = weighted_scores(feats, members, w)
        excluded = ([int(r) for r in rows] if rows is not None else []) + [int(e) for e in (excl or [])]
        self.want = expected_where(cache[key], feats, where, excluded, self.topn)

    def run(self, obj):
        return call_padded(obj, self.rows, self.vecs, self.weights, self.excl, self.where, self.topn)


def playlist_calls(feats, seed, node: bool = False, ks=KS):
    """The calls made on every handle over `feats` (a ramped catalogue), in a fixed order.  Every value of every axis of the
    issue's list occurs on every handle: topn x exclusion list in full, with the members (k, by row / by value), the weights
    and the filter drawn per call; then members x weights in full; then the degenerate calls."""
    n = feats.shape[0]
    rng = np.random.default_rng([seed, n])
    flt = filters(feats)
    excls = exclusion_lists(n, node)
    if n >= BIG:
        ks = tuple(k for k in ks if k <= 3)
    km = []                                                    # (k, rows or None, vecs or None)
    for k in ks:
        rows, vecs = members_of(rng, feats, k)
        km += [(k, rows, None), (k, None, vecs)]
    wk = {}                                                    # weights per k: none and the three weight_kinds
    for k in set(len(m[1]) if m[1] is not None else m[0] for m in km):
        wk[k] = [("unweighted", None)] + list(weight_kinds(rng, k))
    cache = {}

    def make(what, mi, wi, ex_name, f_name, topn):
        k, rows, vecs = km[mi]
        kk = len(rows) if rows is not None else k
        w_name, w = wk[kk][wi]
        return Call(f"n={n} {what}: k={kk} {'by row' if rows is not None else 'by value'}, {w_name}, excl {ex_name}, filter {f_name}, top-{topn}",
                    feats, rows, vecs, w, excls[ex_name], flt[f_name], topn, cache, (mi, wi))

    calls = []
    # (a) topn x exclusion list, the members, the weights and the filter DRAWN per call (half of the calls unfiltered); the
    # everything-excluded list and the nothing filter come in (c): they answer nothing
    for ex_name in [e for e in excls if e != "all"]:
        for t in TOPNS + ("eff-1", "eff", "eff+1"):
            mi, wi = int(rng.integers(0, len(km))), int(rng.integers(0, 4))
            f_name = ("none", "none", "WHERE", "tail3")[int(rng.integers(0, 4))]
            if isinstance(t, str):
                t = n - _n_excluded(n, km[mi][1], excls[ex_name]) + {"eff-1": -1, "eff": 0, "eff+1": 1}[t]
            if 1 <= t <= MAX_TOPN:
                calls.append(make("topn x excl", mi, wi, ex_name, f_name, t))
    # (b) members x weights, the filters and lists in turn
    ex_names = [e for e in excls if e != "all"]
    for j, (mi, wi) in enumerate(itertools.product(range(len(km)), range(4))):
        calls.append(make("members x weights", mi, wi, ex_names[j % len(ex_names)], ("WHERE", "none", "tail3")[j % 3], (10, 257, 3)[j % 3]))
    # (c) the degenerate ones: a filter that admits nothing; everything excluded, and the call after it; a pair that cancels
    # ... and the full answers at the edges, whatever (a) drew: top-256 (the kPlBoundRows side that may start from the anchors'
    # threshold) and topn = eff, eff - 1 (exactly one row dropped) without a filter, by row and by value
    for mi in (2 if len(km) > 2 else 0, 3 if len(km) > 3 else 1):
        for ex_name in ("none", "few"):
            avail = n - _n_excluded(n, km[mi][1], excls[ex_name])
            for t in (256, avail, avail - 1):
                if 1 <= t <= MAX_TOPN:
                    calls.append(make("unfiltered edge", mi, 0, ex_name, "none", t))
    calls.append(make("nothing admitted", len(km) - 1, 0, "few", "nothing", 10))
    calls.append(make("tail quad", 1, 0, "none", "tail3", 10))
    if "all" in excls:
        for mi in (0, 1):
            calls.append(make("everything excluded", mi, 0, "all", "none", 10))
            calls.append(make("the call after", mi, 1, "few", "none", 10))
    a = km[1][2][:1]
    calls.append(Call(f"n={n} cancelling pair (|u| = 0)", feats, None, np.concatenate([a, a]), np.array([1.0, -1.0], np.float32), None, None,
                      10, cache, "cancel"))
    if n >= BIG:                                               # the one k = 32 call of the large sizes
        rows, _ = members_of(rng, feats, 32)
        calls.append(Call(f"n={n} k=32 by row, top-10", feats, rows, None, None, excls["few"], None, 10, cache, "k32"))
    return calls


def unramped_calls(feats, seed, node: bool = False):
    """A short list for the hostile kinds WITHOUT the ramp (it breaks their exact ties and duplicates): k = 3 by row and by
    value, with and without diverse_oracle.WHERE, top-10 and top-257, unweighted and with a dislike."""
    n = feats.shape[0]
    rng = np.random.default_rng([seed, n, 5])
    rows, vecs = members_of(rng, feats, 3)
    excl = exclusion_lists(n, node)["few"]
    cache, calls = {}, []
    for mi, (r, v) in enumerate(((rows, None), (None, vecs))):
        kk = len(r) if r is not None else 3
        for wi, w in enumerate((None, np.where(np.arange(kk) % 3 == 2, -0.5, 1.0).astype(np.float32))):
            for where, topn in ((None, 10), (WHERE, 257), (None, 257), (WHERE, 10)):
                calls.append(Call(f"n={n} without the ramp: k={kk} {'by row' if r is not None else 'by value'}, weights {wi}, "
                                  f"filter {'WHERE' if where else 'none'}, top-{topn}", feats, r, v, w, excl, where, topn, cache, (mi, wi)))
    return calls


def counter_calls(feats, seed):
    """(unfiltered call, filtered call) for the rows_exact checks: k = 3 BY VALUE, top-10, nothing excluded — so that
    eff = min(10, n) > 0 and a scan is launched at every size, n = 1, 2, 3 included (there the tail mask is the whole scan)."""
    n = feats.shape[0]
    rng = np.random.default_rng([seed, n, 7])
    _, vecs = members_of(rng, feats, 3)
    cache = {}
    return (Call(f"n={n} counter, no filter", feats, None, vecs, None, None, None, 10, cache, 0),
            Call(f"n={n} counter, WHERE", feats, None, vecs, None, None, WHERE, 10, cache, 0))


# ---- the raw calls: the result, its count and the padding past it ---------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def call_padded(obj, rows, vecs, weights, excl, where, topn, lam=None, pool=None):
    """One playlist / diversified call through the entry point the engine wrappers would choose (CosineEngine, a lane or
    NodeEngine), with the output buffers filled with 7s first: asserts count in [0, topn] and -1 / +0.0 (/ +0.0) past it,
    returns (ids, scores) or (ids, scores, mmr) cut to the count."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import CosineEngine, make_filter
    node = not isinstance(obj, CosineEngine)
    stem = ("mi355rec_sharded_query_" if node else "mi355rec_query_") + ("playlist_topn" if rows is not None else "mean_topn")
    members = (np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1)) if rows is not None
               else np.ascontiguousarray(np.asarray(vecs, np.float32).reshape(-1, 12)))
    k = int(members.shape[0])
    ex = np.ascontiguousarray(np.asarray([] if excl is None else list(excl), np.int64).reshape(-1))
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    assert w is None or w.size == k
    flt = make_filter(where) if where is not None else None
    p_ex, p_w, p_flt = (_ptr(ex) if ex.size else None), (_ptr(w) if w is not None else None), (ctypes.byref(flt) if flt is not None else None)
    idx, sc, mm = np.full(topn, 7, np.int64), np.full(topn, 7, np.float32), np.full(topn, 7, np.float32)
    c = ctypes.c_int(-5)
    out = (int(topn), _ptr(idx), _ptr(sc))
    lib, h = obj._lib, obj._h
    if lam is not None:
        rc = getattr(lib, stem + "_diverse")(h, _ptr(members), p_w, k, p_ex, int(ex.size), p_flt, ctypes.c_float(float(lam)), int(pool), *out,
                                             _ptr(mm), ctypes.byref(c))
    elif w is not None:
        rc = getattr(lib, stem + "_weighted")(h, _ptr(members), p_w, k, p_ex, int(ex.size), p_flt, *out, ctypes.byref(c))
    elif flt is not None:
        rc = getattr(lib, stem + "_where")(h, _ptr(members), k, p_ex, int(ex.size), p_flt, *out, ctypes.byref(c))
    else:
        rc = getattr(lib, stem)(h, _ptr(members), k, p_ex, int(ex.size), *out, ctypes.byref(c))
    obj._check(rc) if node else capi.check(rc, h)
    n = c.value
    assert 0 <= n <= topn, f"count {n} for topn {topn}"
    assert np.all(idx[:n] >= 0), "a row id below 0 inside the count"
    assert np.all(idx[n:] == -1), f"ids past the count {n}: {idx[n:][:8]}"
    assert not sc[n:].view(np.uint32).any(), f"scores past the count {n}: {sc[n:][:8]}"
    if lam is None:
        return idx[:n].copy(), sc[:n].copy()
    assert not mm[n:].view(np.uint32).any(), f"mmr past the count {n}: {mm[n:][:8]}"
    return idx[:n].copy(), sc[:n].copy(), mm[:n].copy()


def labels_padded(obj, query_row, query_vec, exclude, wanted, topn):
    """One label-filtered call (by row: query_row; by value: query_vec and exclude), buffers filled with 7s first."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import CosineEngine
    node = not isinstance(obj, CosineEngine)
    prefix = "mi355rec_sharded_query_" if node else "mi355rec_query_"
    lab = np.ascontiguousarray(np.asarray(list(wanted), np.int32).reshape(-1))
    idx, sc = np.full(topn, 7, np.int64), np.full(topn, 7, np.float32)
    c = ctypes.c_int(-5)
    tail = (_ptr(lab), int(lab.size), int(topn), _ptr(idx), _ptr(sc), ctypes.byref(c))
    if query_vec is None:
        rc = getattr(obj._lib, prefix + "row_topn_labels")(obj._h, int(query_row), *tail)
    else:
        q = np.ascontiguousarray(np.asarray(query_vec, np.float32).reshape(12))
        rc = getattr(obj._lib, prefix + "topn_labels")(obj._h, _ptr(q), int(exclude), *tail)
    obj._check(rc) if node else capi.check(rc, obj._h)
    n = c.value
    assert 0 <= n <= topn, f"count {n} for topn {topn}"
    assert np.all(idx[n:] == -1) and not sc[n:].view(np.uint32).any(), f"padding past the count {n}"
    return idx[:n].copy(), sc[:n].copy()


# ---- 2. labels ------------------------------------------------------------------------------------------------------------
LABEL_ROWS = 8193
LABEL_RUNS = {0: 513, 1: 1, 2: 0, 31: 63, 32: 64, 33: 0, 100: 2, 500: 65, 700: 0, 1000: 511, 1022: 512, 1023: 1025}
LABEL_ROWS_SMALL = 65
LABEL_RUNS_SMALL = {0: 1, 1: 2, 2: 0, 31: 0, 32: 5, 500: 40, 1022: 1, 1023: 3}
assert sorted(set(LABEL_RUNS.values())) == [0, 1, 2, 63, 64, 65, 511, 512, 513, 1025]


def labelled_catalogue(n: int, runs, seed: int = SEED):
    """A uniform catalogue (a zero row and copies inside) whose label histogram is `runs` {label: rows}, the rows of every
    label scattered over the catalogue (lab_rows is a real permutation), the rest unlabelled (-1)."""
    from oracle import oracle
    feats = oracle.mt19937_uniform(seed % 100_000 + n, n)
    rng = np.random.default_rng([seed, n, 2])
    labels = np.full(n, -1, np.int32)
    where = rng.permutation(n)
    at = 0
    for lab, count in runs.items():
        labels[where[at:at + count]] = lab
        at += count
    assert at <= n
    if n > 20:
        feats[3] = 0.0
        feats[7:10] = feats[6]
    return np.ascontiguousarray(feats), labels


def label_selections(runs):
    """{name: wanted labels}."""
    populated = [lab for lab, c in runs.items() if c > 0]
    empty = [lab for lab, c in runs.items() if c == 0]
    sel = {f"label {lab}": [lab] for lab in populated}
    sel["1022 and 1023"] = [1022, 1023]
    sel["all 1024"] = list(range(1024))
    sel["only empty"] = empty + [999]
    sel["empty and populated"] = [empty[0], populated[2], empty[1], populated[-2], 999, populated[-1]]
    sel["duplicates"] = [1023, populated[0], 1023, populated[0]]
    return sel


def label_topns(selected: int):
    return sorted({t for t in (1, 10, selected - 1, selected, selected + 5, 1024, 1500) if t >= 1})


def label_queries(labels, wanted):
    """(by-row queries: inside and outside the selection; by-value exclusions: -1 and a selected row)."""
    member = np.isin(labels, wanted)
    inside, outside = np.flatnonzero(member), np.flatnonzero(~member)
    by_row = ([int(inside[0]), int(inside[-1])] if inside.size else []) + ([int(outside[len(outside) // 2])] if outside.size else [])
    by_value = [-1] + ([int(inside[inside.size // 2])] if inside.size else [])
    return by_row, by_value


# ---- 3. diversified top-N on small pools ----------------------------------------------------------------------------------
DIVERSE_SIZES = (1, 2, 5, 63, 64, 65, 257, 1023, 1024, 1025, 4097)
DIVERSE_POOLS = ("topn", 64, 65, 1024)
DIVERSE_TOPNS = (1, 10, 64, 65, 256)
NODE_SIZES = (5, 257, 4097)
FETCH_SIZES = (1, 63, 65)


def diverse_grid():
    """(topn, pool) with pool >= topn."""
    out = []
    for topn in DIVERSE_TOPNS:
        for pool in DIVERSE_POOLS:
            pool = topn if pool == "topn" else pool
            if pool >= topn and (topn, pool) not in out:
                out.append((topn, pool))
    return out


def small_variants(rng, feats, k):
    """diverse_oracle.variants with its 300 excluded ids cut to a quarter of a small catalogue (they would empty it)."""
    n = feats.shape[0]
    for name, rows, vecs, w, excl, where in diverse_variants(rng, feats, min(k, n)):
        if excl is not None and n < 1200:
            excl = excl[:max(1, n // 4)]
        yield name, rows, vecs, w, excl, where


def diverse_cases(feats, seed, k: int = 3):
    """[(what, variant, lam, pool, topn, want)]: every (topn, pool) for every variant; all of LAMBDAS for the first two
    variants, two of them in turn for the others.  The oracle's pool is computed once per variant."""
    from tests.diverse_oracle import variant_pool
    n = feats.shape[0]
    rng = np.random.default_rng([seed, n, 3])
    out = []
    for vi, v in enumerate(small_variants(rng, feats, k)):
        pidx, prel = variant_pool(feats, v, 1024)                  # a smaller pool is a prefix of it (canonical order)
        for gi, (topn, pool) in enumerate(diverse_grid()):
            lams = LAMBDAS if vi < 2 else (LAMBDAS[(gi + vi) % 5], LAMBDAS[(gi + vi + 2) % 5])
            for lam in lams:
                out.append((f"n={n} {v[0]} top-{topn} pool {pool} lambda {lam}", v, lam, pool, topn, rerank(feats, pidx[:pool], prel[:pool], lam, topn)))
    return out


def run_diverse(obj, v, lam, pool, topn):
    name, rows, vecs, w, excl, where = v
    return call_padded(obj, rows, vecs, w, excl, where, topn, lam=lam, pool=pool)


def copies_catalogue():
    """1024 copies of one row plus one other row (the last): by value against the copied row every relevance and every
    penalty ties, so the picks come in pool order, across all 16 waves."""
    rng = np.random.default_rng(SEED + 1)
    f = np.tile(rng.random((1, 12), dtype=np.float32), (1025, 1))
    f[1024] = rng.random(12, dtype=np.float32)
    return np.ascontiguousarray(f)


def half_zero_catalogue(n: int = 1023):
    """Every even row zero."""
    f = np.random.default_rng(SEED + 2).random((n, 12), dtype=np.float32)
    f[::2] = 0.0
    return np.ascontiguousarray(f)


# ---- the case lists as the suites take them: generated once per process, whichever test asks first ------------------------
DIVERSE_KINDS = (0, 6, 2, 5, 4, 1, 3)     # the kind of DIVERSE_SIZES[i] is DIVERSE_KINDS[i % 7]


def sweep_catalogues(cpu: bool):
    """[(n, kind)] of section 1: every size with its kinds; the CPU leg sizes up to CPU_MAX_ROWS, plain and hostile in turn."""
    if not cpu:
        return [(n, kind) for n in SIZES for kind in kinds_at(n)]
    sizes = [n for n in SIZES if n <= CPU_MAX_ROWS]
    return [(n, kinds_at(n)[i % 2]) for i, n in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def catalogue_cases(n: int, kind: int, node: bool):
    """(catalogue, its ramped copy, the calls on the ramped copy, the calls on the catalogue itself — hostile kinds only —,
    the two counter calls)."""
    feats = catalogue_of_kind(kind, n)
    fr = ramped(feats)
    more = tuple(unramped_calls(feats, SEED + kind, node)) if kind in HOSTILE_KINDS else ()
    return feats, fr, tuple(playlist_calls(fr, SEED + kind, node)), more, counter_calls(fr, SEED + kind)


@functools.lru_cache(maxsize=None)
def diverse_catalogue(n: int):
    """(kind, catalogue, diverse_cases) of one of DIVERSE_SIZES."""
    kind = DIVERSE_KINDS[DIVERSE_SIZES.index(n) % 7]
    feats = catalogue_of_kind(kind, n)
    return kind, feats, tuple(diverse_cases(feats, SEED + kind))


@functools.lru_cache(maxsize=None)
def crafted_diverse():
    """{name: (catalogue, [(what, variant, lam, pool, topn, want)])}: the copies (by value against the copied row, every
    relevance and penalty ties: the oracle itself must pick in pool order) and the half-zero catalogue."""
    from tests.diverse_oracle import expected
    f = copies_catalogue()
    v = ("by value against the copied row", None, f[:1], None, None, None)
    copies = []
    for lam in LAMBDAS:
        for topn, pool in ((256, 1024), (65, 65), (1024, 1024)):
            want = expected(f, f[:1], None, [], None, lam, pool, topn)
            assert want[0].tolist() == list(range(topn)), "the oracle itself: every value ties, pool order"
            copies.append((f"lambda {lam} top-{topn} pool {pool}", v, lam, pool, topn, want))
    h = half_zero_catalogue()
    return {"1024 copies and one row": (f, tuple(copies)), "half zero rows": (h, tuple(diverse_cases(h, SEED + 9)))}


def empty_share(cpu: bool):
    """(cases with an empty expected answer, cases) over the playlist and diversified cases of a suite, from the oracles'
    answers alone: it does not depend on which tests ran, or in which order."""
    wants = []
    for n, kind in sweep_catalogues(cpu):
        _, _, calls, more, _ = catalogue_cases(n, kind, cpu)
        wants += [c.want for c in calls + more]
    for n in DIVERSE_SIZES:
        if not cpu or n <= CPU_MAX_ROWS:
            wants += [c[-1] for c in diverse_catalogue(n)[2]]
    for _, todo in crafted_diverse().values():
        wants += [c[-1] for c in todo]
    return sum(int(len(w[0]) == 0) for w in wants), len(wants)


def label_sweep(obj, feats, labels, selections, what):
    """Every selection: by row from inside and outside it, by value with nothing and with a selected row excluded, every
    topn of label_topns — against labels_oracle.expected_from_scores, count and padding included."""
    from oracle import oracle
    from tests.labels_oracle import check, expected_from_scores
    vec = np.random.default_rng(SEED).random(12, dtype=np.float32)
    vec_scores = oracle.scores(feats, vec)
    for name, wanted in selections.items():
        selected = int(np.isin(labels, wanted).sum())
        by_row, by_value = label_queries(labels, wanted)
        for q in by_row:
            scores = oracle.scores(feats, feats[q])
            for topn in label_topns(selected):
                want = expected_from_scores(scores, labels, q, wanted, topn)
                check(labels_padded(obj, q, None, -1, wanted, topn), want, f"{what} {name} row {q} top-{topn}")
        for excl in by_value:
            for topn in label_topns(selected):
                want = expected_from_scores(vec_scores, labels, excl, wanted, topn)
                assert len(want[0]) == min(topn, selected - (1 if excl >= 0 else 0))
                check(labels_padded(obj, -1, vec, excl, wanted, topn), want, f"{what} {name} by value, exclude {excl}, top-{topn}")
