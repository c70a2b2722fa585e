"""The cases of the node-handle sweep over short and empty shards (tests/test_gpu_node_sweep.py on the MI355X over virtual shards
`devices=[0] * shards`, tests/test_node_sweep_cpu.py for the case definitions themselves): the (rows, shards) geometries, the
catalogue and side data built for them, the request matrix, and every case's expectation from the oracles the suite already has.

A case is a kind, a spec (plain values: members by row or by value, topn, the options) and two functions of it: `expect` asks
the kind's oracle, `run` makes the call on an engine object (a NodeEngine of any placement, or a CosineEngine over the same
catalogue) through the padded raw calls of the oracles' own request_call helpers, so the count and the -1 / 0.0 past it are
checked with every call.  Everything is compared bit for bit; there is no tolerance in this file.

Every restriction of a request (exclusion list, members given by row, filter, label set, row set, candidate list) is turned into
ONE exclusion list here (`structural`), and the oracles, which take exclusion lists of any length, are asked with it: the
expectation of a composed request is then the oracle's, not a second implementation's.

What the interface rules out, so no case holds it:
  * a node handle refuses an excluded id >= n (ERR_INVALID_ARG, "excluded row ... out of the catalogue") where the single handle
    lets it match nothing: the matrix's exclusion lists stay below n, `foreign_exclusions` holds the list with ids >= n that the
    GPU leg gives to the single handle and sees refused by the node;
  * pool and topn are at most 1024, so "a pool larger than a shard's rows" ends at shards of 1025 rows and more.

Where every shard holds one row, a tied pair on BOTH sides of EVERY edge makes the whole catalogue one row repeated.  That
catalogue is kept (variant "tied": every answer is decided by the row ids alone, across up to 64 lists), and the geometries it
happens to get a second one, "alternate", with a pair at every other edge, so that scores still differ between shards there."""
import contextlib
import ctypes
import functools

import numpy as np

SEED = 20261021
F32 = np.float32

# (rows, shards): what each puts on a shard, and the branch it is there for, is the table of DESIGN.md §5.4.25
GEOMETRIES = ((1, 3), (2, 2), (3, 3), (5, 8), (13, 3), (37, 5), (67, 8), (131, 16), (259, 3), (1031, 7), (2051, 2), (4099, 2),
              (4099, 5), (70, 64))
WIDE = (70, 64)                                   # MI355REC_MAX_SHARDS: its own test, three kinds
ALTERNATE = ((3, 3), (5, 8), (70, 64))            # the geometries whose "tied" catalogue is one row repeated
CATALOGUES = tuple((n, g, "tied") for n, g in GEOMETRIES) + tuple((n, g, "alternate") for n, g in ALTERNATE)
TOPNS = (1, 10, 100, 1024)
EMBED_GEOMETRIES = ((5, 8), (37, 5), (1031, 7))
EMBED_DIMS = (16, 64)

L_ONE, L_ALL, L_ABSENT, L_NONE = 2, 5, 9, 777     # a label of one shard, the common one, one that a shard lacks, one no row has
FEW = {11: (0.7, 0.8)}                            # the filter that admits two or three rows of a shard (feature 11 is built for it)
BAND = {0: (0.2, 0.8)}
SCALES = np.array([2, 1, .5, 0, 1, 1, 3, 1, .25, 1, 1, 0], F32)   # (tests/scaled_oracle.GENERAL)
KINDS = ("cosine", "distance", "manhattan", "jaccard", "anyof", "bounded", "diverse", "capped", "candidates", "scores", "labels1")
WIDE_KINDS = ("cosine", "bounded", "anyof")


def bounds(n: int, g: int):
    from spotify_recommender_amd.engine import shard_bounds
    return [shard_bounds(n, g, r) for r in range(g)]


class Catalogue:
    """The rows, the side data and the rows the requests are made of, for one (rows, shards, variant)."""

    def __init__(self, n, g, variant):
        self.n, self.g, self.variant = n, g, variant
        self.bounds = bounds(n, g)
        self.sizes = [hi - lo for lo, hi in self.bounds]
        self.shard = np.repeat(np.arange(g), self.sizes)                      # the shard of every row
        self.nonempty = [r for r in range(g) if self.sizes[r] > 0]
        self.cache = {}
        rng = np.random.default_rng([SEED, n, g])
        f = (rng.random((n, 12), dtype=F32) * F32(0.8) + F32(0.1)).astype(F32)
        base = (rng.random(12, dtype=F32) * F32(0.8) + F32(0.1)).astype(F32)
        base[11] = F32(0.25)                                                  # (feature 11 is the FEW filter's: see below)
        # the standard request: three members close to one direction; the short shard's rows lie along it
        self.std = np.ascontiguousarray(np.clip(np.stack([base, base * F32(1.01) + F32(0.01) * rng.random(12, dtype=F32),
                                                          base * F32(0.99) + F32(0.01) * rng.random(12, dtype=F32)]), 0, 1).astype(F32))
        self.far = np.where(base > np.median(base), F32(0.02), F32(0.95)).astype(F32)   # a direction away from it
        self.short = self.nonempty[-1] if len(self.nonempty) >= 2 else None             # (the last non-empty shard is a smallest one)
        self.starved = self.nonempty[len(self.nonempty) // 2 - (len(self.nonempty) % 2 == 0)] if len(self.nonempty) >= 3 else None
        if self.short is not None:
            lo, hi = self.bounds[self.short]
            for r in range(lo, min(hi, lo + 9)):                              # (at most nine of them: a large shard keeps its other rows)
                f[r] = np.clip(base + F32(0.002) * rng.random(12, dtype=F32), 0, 1)
        if self.starved is not None:
            lo, hi = self.bounds[self.starved]
            for r in range(lo, hi):
                f[r] = np.clip(self.far + F32(0.02) * rng.random(12, dtype=F32), 0, 1)
        # feature 11: 0.75 on two or three rows of a shard (FEW admits them), 0.25 elsewhere
        f[:, 11] = F32(0.25)
        for s in self.nonempty:
            lo, size = self.bounds[s][0], self.sizes[s]
            few = [lo + 1, lo + 2] + ([lo + 3] if size >= 6 else []) if size >= 4 else ([lo + size - 1] if s % 2 == 0 else [])
            f[few, 11] = F32(0.75)
        # bit-identical copies on both sides of a shard edge ("tied": every edge; "alternate": every edge that shares no row with
        # the pair before it)
        self.pairs, used = [], -1
        for s in self.nonempty[1:]:
            e = self.bounds[s][0]
            if variant == "alternate" and e - 1 <= used:
                continue
            f[e] = f[e - 1]
            self.pairs.append((e - 1, e))
            used = e
        paired = {r for p in self.pairs for r in p}
        # the hostile VALUES of make_catalogue's kind 6 (tests/test_gpu_fuzz.py), away from the edges and from the short and the
        # starved shard (the oracle's score of a row with an infinite feature is 1.0)
        inner = [r for r in range(n) if r not in paired and self.shard[r] not in (self.short, self.starved)
                 and f[r, 11] == F32(0.25) and 0 < r - self.bounds[self.shard[r]][0] < self.sizes[self.shard[r]] - 1]
        self.hostile = []
        if n >= 13 and len(inner) >= 12:
            self.hostile = [int(r) for r in rng.choice(inner, size=6, replace=False)]
            z, a, b, c, d, e = self.hostile
            f[z] = 0.0
            f[a, 3], f[b, 5], f[c, 7], f[d, 2], f[e, 9] = np.nan, np.inf, -np.inf, F32(1e-42), F32(3e19)
        self.feats = np.ascontiguousarray(f)
        self._side_data(rng)
        self._request_rows(rng, paired)

    def _side_data(self, rng):
        n = self.n
        lab = np.full(n, L_ALL, np.int32)
        first, last = self.nonempty[0], self.nonempty[-1]
        for s in self.nonempty:
            lo, size = self.bounds[s][0], self.sizes[s]
            if s != last or len(self.nonempty) == 1:
                if size >= 2:
                    lab[lo + size // 2] = L_ABSENT
                elif s % 2 == 1:
                    lab[lo] = L_ABSENT
        lo, size = self.bounds[first][0], self.sizes[first]
        lab[lo + size - 1 if size >= 3 else lo] = L_ONE                       # L_ONE: rows of the first shard only
        if size >= 5:
            lab[lo + 1] = -1
        self.labels = lab
        pri = ((rng.random(n, dtype=F32) * F32(2) - F32(1)) * F32(0.9)).astype(F32)
        ones = [s for s in self.nonempty if self.sizes[s] == 1]
        pri[self.bounds[ones[-1] if ones else self.nonempty[-1]][0]] = F32(1.0)   # the largest prior on a one-row shard, where there is one
        self.priors = pri
        grp = (np.arange(n) % 4 + 1).astype(np.int32)
        grp[np.arange(n) % 11 == 5] = -1
        for s in self.nonempty:
            grp[self.bounds[s][0]] = 0                                        # group 0 has a row on every shard
        self.groups = grp

    def _request_rows(self, rng, paired):
        n = self.n
        plain = [r for r in range(n) if r not in self.hostile]
        calm = [r for r in plain if r not in paired and (self.short is None or self.shard[r] != self.short)] or plain
        k = min(3, max(1, n // 4))
        shards = sorted({self.shard[r] for r in calm})
        take = [shards[i * (len(shards) - 1) // max(k - 1, 1)] for i in range(k)] if len(shards) >= k else shards
        self.mrows = []
        for s in dict.fromkeys(take):                                         # members from different shards
            rows = [r for r in calm if self.shard[r] == s]
            self.mrows.append(int(rows[len(rows) // 2]))
        self.mrows = (self.mrows + [r for r in calm if r not in self.mrows])[:k]
        self.k32 = [int(r) for r in rng.choice(plain, size=min(32, max(1, n - 2), len(plain)), replace=False)]
        pool = sorted({int(r) for r in plain[::4]} | {r for p in self.pairs[:2] for r in p if r in plain})[:max(1, n // 4)]
        self.x1024 = [int(pool[i]) for i in rng.integers(0, len(pool), size=1024)]   # MI355REC_MAX_EXCLUDE entries, few distinct
        several = [r for p in self.pairs[:1] for r in p] + [self.bounds[s][0] for s in self.nonempty[:3]] + [n - 1, n - 1]
        self.several = [int(r) for r in several if n > 2] or [0]
        self.seen = [int(r) for r in np.flatnonzero(rng.random(n) < 0.3)] or [0]
        self.only = [int(r) for r in range(0, n, 2)]
        # any-of: member 2 is member 0 bit for bit (a tie between members: index 0 is reported), member 1 matches the starved shard,
        # member 3 is a row of the first shard (the short shard's rows match member 0)
        self.any_vecs = np.ascontiguousarray(np.stack([self.std[0], self.far, self.std[0], self.feats[calm[0]]]).astype(F32))
        pair_rows = [r for p in self.pairs[:1] for r in p if r in plain]
        self.any_rows = (pair_rows + [r for r in self.mrows if r not in pair_rows])[:max(1, min(3, n - 1))] if n > 3 else self.mrows
        self.l1_vecs = np.ascontiguousarray((rng.random((11, 12), dtype=F32) * F32(0.8) + F32(0.1)).astype(F32))

    def lists(self):
        """{name: candidate ids}: every id in one shard; none in some shard; duplicates; descending; everything; nothing."""
        n = self.n
        lo, hi = self.bounds[self.nonempty[0]]
        miss = self.nonempty[-1] if len(self.nonempty) > 1 else None
        out = {"one shard": list(range(lo, min(hi, lo + 50))),
               "none in a shard": [r for r in range(n) if miss is None or self.shard[r] != miss][::max(1, n // 300)],
               "duplicates": [0, n - 1, 0, n // 2, n - 1, n // 2, 0],
               "descending": list(range(n - 1, -1, -max(1, n // 200))),
               "everything": list(range(n)),
               "nothing": []}
        if miss is not None and len(self.nonempty) == 2:      # (two shards: "none in a shard" is "one shard"; keep the other shard's rows too)
            out["none in a shard"] = out["none in a shard"][:200]
        return out

    def updated(self):
        """(rows, their new features, the catalogue after it): rows on both sides of every shard edge but those of one shard, which
        stays untouched (three non-empty shards and more), a one-row shard among them where there is one; some new rows tie."""
        rng = np.random.default_rng([SEED, self.n, self.g, 6])
        keep = self.nonempty[1] if len(self.nonempty) >= 3 else None
        rows = []
        for s in self.nonempty[1:]:
            e = self.bounds[s][0]
            for r in (e - 1, e):
                if self.shard[r] != keep and r not in rows:
                    rows.append(int(r))
        rows = rows or [0]
        new = (rng.random((len(rows), 12), dtype=F32) * F32(0.8) + F32(0.1)).astype(F32)
        new[:, 11] = self.feats[rows, 11]
        if len(rows) >= 4:
            new[-1] = new[0]                                                  # a tie between rows of distant shards
            new[1] = self.std[0]
        rows = rows[::-1]                                                     # (any order)
        new = np.ascontiguousarray(new[::-1])
        after = Catalogue.__new__(Catalogue)
        after.__dict__.update(self.__dict__)
        after.cache = {}
        after.feats = self.feats.copy()
        after.feats[rows] = new
        return rows, new, after


@functools.lru_cache(maxsize=None)
def catalogue(n: int, g: int, variant: str = "tied") -> Catalogue:
    return Catalogue(n, g, variant)


# ---- a case: its kind and its spec --------------------------------------------------------------------------------------------
class Case:
    def __init__(self, kind, what, **spec):
        self.kind, self.what, self.spec = kind, what, spec
        self.want = self.adm = None

    def get(self, key, default=None):
        return self.spec.get(key, default)

    @property
    def ids(self):
        """The rows of the expected answer (candidate scores: the listed rows that get a value)."""
        if self.kind == "scores":
            return np.asarray(self.get("cand"), np.int64)[self.want[1]]
        return np.asarray(self.want[0], np.int64)

    @property
    def empty(self):
        return self.want[2] == 0 if self.kind == "bounded" else self.ids.size == 0


def _members(cat, c):
    rows = c.get("rows")
    return cat.feats[[int(r) for r in rows]] if rows is not None else np.asarray(c.get("vecs"), F32).reshape(-1, 12)


def structural(cat, c, listed=True):
    """The rows the request's restrictions leave (before what the kind's values rule out): not excluded, no member given by row,
    inside the filter, the label set, the row set and (listed) the candidate list."""
    from tests.filter_oracle import pass_mask
    n = cat.n
    ok = np.ones(n, bool)
    for e in list(c.get("exclude") or []) + list(c.get("rows") or []):
        if 0 <= int(e) < n:
            ok[int(e)] = False
    if c.get("where") is not None:
        ok &= pass_mask(cat.feats, c.get("where"))
    if c.get("wanted") is not None:
        ok &= np.isin(cat.labels, np.asarray(list(c.get("wanted")), np.int64)) & (cat.labels >= 0)
    if c.get("rowset") is not None:
        ids, mode = c.get("rowset")
        inside = np.zeros(n, bool)
        inside[np.asarray(ids, np.int64)] = True
        ok &= inside if mode == "only" else ~inside
    if listed and c.get("cand") is not None:
        inside = np.zeros(n, bool)
        inside[np.asarray(c.get("cand"), np.int64)] = True
        ok &= inside
    return ok


def _cached(cat, key, make):
    if key not in cat.cache:
        cat.cache[key] = make()
    return cat.cache[key]


def _mkey(c):
    rows = c.get("rows")
    return ("rows", tuple(int(r) for r in rows)) if rows is not None else ("vecs", np.asarray(c.get("vecs"), F32).tobytes())


def _cosine_values(cat, c):
    from tests import prior_oracle, scaled_oracle
    from tests.playlist_labels_oracle import scores_of
    w = c.get("weights")
    key = ("cos", _mkey(c), None if w is None else tuple(float(x) for x in w), c.get("scales") is not None)
    members = _members(cat, c)
    s = _cached(cat, key, lambda: scaled_oracle.cosine_scores(cat.feats, members, c.get("scales"), w) if c.get("scales") is not None
                else scores_of(cat.feats, members, w))
    return s if c.get("prior") is None else prior_oracle.blended(s, cat.priors, c.get("prior"))


def _distance_m(cat, c):
    from tests import distance_oracle, scaled_oracle
    members = _members(cat, c)
    return _cached(cat, ("m2", _mkey(c), c.get("scales") is not None),
                   lambda: scaled_oracle.distance_m(cat.feats, members, c.get("scales")) if c.get("scales") is not None
                   else distance_oracle.mean_sqdist(cat.feats, members))


def expect(cat, c):
    """Sets c.want (what the kind's check compares with) and c.adm (the rows that may be returned at all)."""
    from oracle import oracle
    from tests import (anyof_oracle, bounded_oracle, candidate_scores_oracle, capped_oracle, distance_oracle, diverse_oracle,
                       jaccard_oracle, labels_oracle, manhattan_oracle)
    from tests.playlist_oracle import expected_from_scores
    kind, topn = c.kind, c.get("topn")
    if kind == "labels1":
        row, excl = c.get("qrow"), c.get("qexcl", -1)
        q = cat.feats[row] if row is not None else np.asarray(c.get("qvec"), F32)
        excl = row if row is not None else excl
        scores = _cached(cat, ("single", q.tobytes()), lambda: oracle.scores(cat.feats, np.ascontiguousarray(q)))
        c.want = labels_oracle.expected_from_scores(scores, cat.labels, excl, c.get("wanted"), topn)
        c.adm = np.isin(cat.labels, np.asarray(list(c.get("wanted")), np.int32)) & (np.arange(cat.n) != excl)
        return c
    ok = structural(cat, c)
    gone = np.flatnonzero(~ok)
    members = _members(cat, c)
    if kind in ("cosine", "diverse", "capped") or (kind in ("candidates", "scores") and c.get("metric") == "cosine"):
        s = _cosine_values(cat, c)
        c.adm = ok
        if kind == "scores":
            c.want = candidate_scores_oracle.expected(cat.n, c.get("cand"), s, np.flatnonzero(~structural(cat, c, listed=False)))
        elif kind == "diverse":
            pidx, prel = expected_from_scores(s, gone, c.get("pool"))
            c.want = diverse_oracle.rerank(cat.feats, pidx, prel, c.get("lam"), topn) if pidx.size else (pidx, prel, prel.copy())
        elif kind == "capped":
            pidx, prel = expected_from_scores(s, gone, c.get("pool"))
            picks = capped_oracle.rerank_capped(cat.feats, pidx, prel, cat.groups, c.get("lam"), c.get("mpg"), topn) if pidx.size \
                else (pidx, prel, prel.copy())
            c.want = picks + (int(pidx.size),)
        else:
            c.want = expected_from_scores(s, gone, topn)
    elif kind in ("distance", "candidates", "scores"):
        m = _distance_m(cat, c)
        c.adm = ok & np.isfinite(m)
        if kind == "scores":
            c.want = candidate_scores_oracle.expected(cat.n, c.get("cand"), m, np.flatnonzero(~structural(cat, c, listed=False)), distance=True)
        else:
            c.want = distance_oracle.expected_from_m(cat.feats, m, gone, topn)
            if c.get("ids_only"):
                c.want = (c.want[0],)
    elif kind == "manhattan":
        m = _cached(cat, ("m1", _mkey(c)), lambda: manhattan_oracle.mean_l1(cat.feats, members))
        c.adm = ok & np.isfinite(m)
        c.want = manhattan_oracle.expected_from_m(cat.feats, m, gone, topn)
        if c.get("ids_only"):
            c.want = (c.want[0],)
    elif kind == "jaccard":
        v, valid = _cached(cat, ("jac", _mkey(c)), lambda: jaccard_oracle.mean_jaccard(cat.feats, members))
        c.adm = ok & valid
        c.want = jaccard_oracle.expected_from_v(cat.feats, (v, valid), gone, topn)
    elif kind == "anyof":
        v, a = _cached(cat, ("any", _mkey(c)), lambda: anyof_oracle.value(cat.feats, members))
        c.adm = ok
        c.want = anyof_oracle.expected_from_v(cat.feats, v, a, gone, topn)[:2 if c.get("no_member") else 3]
    elif kind == "bounded":
        metric = bounded_oracle.EUCLIDEAN if c.get("metric") == "euclidean" else bounded_oracle.COSINE
        v = _cached(cat, ("bnd", _mkey(c), metric), lambda: bounded_oracle.values(cat.feats, members, metric))
        okb = bounded_oracle.admissible(cat.feats, v, gone)
        c.want = bounded_oracle.expected_from_values(v, okb, metric, c.get("bound"), topn)
        c.adm = okb & (bounded_oracle.image(v) >= bounded_oracle.image(bounded_oracle.floor_score(metric, c.get("bound"))))
    else:
        raise ValueError(kind)
    return c


def _bits(x):
    x = np.asarray(x)
    return x.astype(F32).view(np.uint32) if x.dtype.kind == "f" else x


def same(a, b) -> bool:
    """Two results of one case, element by element: equal ids, counts and member indices, bit-equal floats."""
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def check(c, got, what=""):
    """The kind's own check of `got` against the oracle's answer."""
    from tests import (anyof_oracle, bounded_oracle, candidate_scores_oracle, capped_oracle, distance_oracle, diverse_oracle,
                       jaccard_oracle, labels_oracle, manhattan_oracle)
    what = f"{what} {c.kind}: {c.what}"
    if c.get("ids_only"):
        assert np.asarray(got[0]).tolist() == np.asarray(c.want[0]).tolist(), f"{what}: ids differ"
        return
    if c.get("no_member"):
        return labels_oracle.check(got, c.want, what)
    {"cosine": labels_oracle.check, "candidates": distance_oracle.check if c.get("metric") == "euclidean" else labels_oracle.check,
     "labels1": labels_oracle.check, "distance": distance_oracle.check, "manhattan": manhattan_oracle.check,
     "jaccard": jaccard_oracle.check, "anyof": anyof_oracle.check, "bounded": bounded_oracle.check, "diverse": diverse_oracle.check3,
     "capped": lambda g, w, t: capped_oracle.check4(g, w[:3], w[3], t), "scores": candidate_scores_oracle.check}[c.kind](got, c.want, what)


def run(eng, c):
    """The case's call on `eng` (NodeEngine or CosineEngine): through the padded raw calls, the handle's own error on a refusal."""
    from spotify_recommender_amd import capi
    from tests import (anyof_oracle, bounded_oracle, candidate_scores_oracle, candidates_oracle, distance_oracle, jaccard_oracle,
                       manhattan_oracle, playlist_labels_oracle, prior_oracle, rowset_oracle, scaled_oracle)
    from tests.playlist_sweep_cases import call_padded, labels_padded
    kind, topn, h = c.kind, c.get("topn"), eng._h

    def fn(name):
        return getattr(eng._lib, eng._prefix + name)

    def done(res):
        eng._check(res[0])
        return tuple(res[1:])

    if kind == "labels1":
        return labels_padded(eng, c.get("qrow"), c.get("qvec"), c.get("qexcl", -1), c.get("wanted"), topn)
    rows, vecs = c.get("rows"), c.get("vecs")
    kw = dict(rows=[int(r) for r in rows]) if rows is not None else dict(members=vecs)
    kw.update(exclude=c.get("exclude"), where=c.get("where"), labels=c.get("wanted"), topn=topn)
    cand, scales, prior, w = c.get("cand"), c.get("scales"), c.get("prior"), c.get("weights")
    with contextlib.ExitStack() as stack:
        rs, mode = None, 0
        if c.get("rowset") is not None:
            rs = stack.enter_context(eng.row_set(c.get("rowset")[0]))._ptr()
            mode = capi.ROWSET_ONLY if c.get("rowset")[1] == "only" else capi.ROWSET_EXCLUDE
        ext = capi.RequestExt(ctypes.sizeof(capi.RequestExt), mode, None, rs) if rs is not None else None
        if kind in ("diverse",) or (kind == "cosine" and not (c.get("wanted") or prior is not None or scales is not None or rs)):
            return call_padded(eng, rows, vecs, w, c.get("exclude"), c.get("where"), topn, lam=c.get("lam"), pool=c.get("pool"))
        if kind == "capped":
            return done(playlist_labels_oracle.request_call(capi, fn("query_playlist_request"), h, weights=w, lam=c.get("lam"),
                                                            pool=c.get("pool"), max_per_group=c.get("mpg"), **kw))
        if kind == "cosine":
            if rs is not None:
                return done(rowset_oracle.request_call(capi, fn("query_playlist_request_ext"), h, "cosine", rs, mode, scales=scales,
                                                       prior_weight=prior, weights=w, **kw))[:2]
            if scales is not None:
                return done(scaled_oracle.request_call(capi, fn("query_playlist_request_scaled"), h, "cosine", scales, weights=w, **kw))
            if prior is not None:
                return done(prior_oracle.request_call(capi, fn("query_playlist_request"), h, prior_weight=prior, weights=w, **kw))[:2]
            return done(playlist_labels_oracle.request_call(capi, fn("query_playlist_request"), h, weights=w, **kw))[:2]
        if kind == "distance":
            if c.get("ids_only"):
                return (_ids_only(eng, "distance", c),)
            if rs is not None:
                return done(rowset_oracle.request_call(capi, fn("query_distance_request_ext"), h, "euclidean", rs, mode, scales=scales, **kw))
            if scales is not None:
                return done(scaled_oracle.request_call(capi, fn("query_distance_request_scaled"), h, "euclidean", scales, **kw))
            return done(distance_oracle.request_call(capi, fn("query_distance_request"), h, **kw))
        if kind == "candidates":
            metric = c.get("metric")
            more = dict(weights=w, prior_weight=prior) if metric == "cosine" else {}
            res = done(candidates_oracle.request_call(capi, fn(f"query_{'playlist' if metric == 'cosine' else 'distance'}_request_candidates"),
                                                      h, metric, cand, rs, mode, scales=scales, **more, **kw))
            return res[:2]
        if kind == "scores":
            metric = c.get("metric")
            more = dict(weights=w, prior_weight=prior) if metric == "cosine" else {}
            val, flags = done(candidate_scores_oracle.score_call(
                capi, fn(f"score_{'playlist' if metric == 'cosine' else 'distance'}_request_candidates"), h, metric, cand, rs, mode,
                scales=scales, **more, **kw))
            return val, flags.astype(bool)
        if kind == "manhattan":
            return done(manhattan_oracle.request_call(capi, fn("query_manhattan_request"), h, ext=ext, want_distance=not c.get("ids_only"), **kw))[
                :1 if c.get("ids_only") else 2]
        if kind == "jaccard":
            return done(jaccard_oracle.request_call(capi, fn("query_jaccard_request"), h, ext=ext, **kw))
        if kind == "anyof":
            res = done(anyof_oracle.request_call(capi, fn("query_anyof_request"), h, ext=ext, want_member=not c.get("no_member"), **kw))
            return res[:2] if c.get("no_member") else res
        if kind == "bounded":
            metric = bounded_oracle.EUCLIDEAN if c.get("metric") == "euclidean" else bounded_oracle.COSINE
            return done(bounded_oracle.request_call(capi, fn("query_bounded_request"), h, metric=metric, bound=c.get("bound"), ext=ext, **kw))
    raise ValueError(kind)


def _ids_only(eng, kind, c):
    """A distance request whose result struct has NO distance pointer: the ids alone, the padding checked."""
    from spotify_recommender_amd import capi
    from spotify_recommender_amd.engine import _fill_query, _np_members, _np_rows
    topn = c.get("topn")
    m = _np_rows(c.get("rows")) if c.get("rows") is not None else _np_members(c.get("vecs"))
    q = capi.DistanceQuery()
    keep = _fill_query(q, m, topn, c.get("exclude"), c.get("where"), c.get("wanted"))   # noqa: F841
    idx, count = np.full(topn, 7, np.int64), ctypes.c_int(-5)
    res = capi.DistanceResult(idx.ctypes.data_as(ctypes.c_void_p), None, ctypes.pointer(count))
    eng._check(getattr(eng._lib, eng._prefix + "query_distance_request")(eng._h, ctypes.byref(q), ctypes.byref(res)))
    assert 0 <= count.value <= topn and np.all(idx[count.value:] == -1), (count.value, idx)
    return idx[:count.value].copy()


# ---- the request matrix -------------------------------------------------------------------------------------------------------
def request_matrix(cat, kinds=KINDS, short=False):
    """Every case of a catalogue, expectations included.  `short`: one case per kind (what is repeated after side data has been
    set again and after update_rows)."""
    from tests import bounded_oracle
    n, std, mrows = cat.n, cat.std, cat.mrows
    pool = min(1024, max(n + 7, 100))                                         # above n (up to 1024) and never below a topn of 100
    out = []

    def add(kind, what, **spec):
        if kind in kinds:
            out.append(Case(kind, f"{what}, top-{spec.get('topn')}", **spec))

    if short:
        add("cosine", "by row, labels, prior, seen", rows=mrows, wanted=[L_ALL, L_ABSENT], prior=0.5, rowset=(cat.seen, "seen"), topn=100)
        add("distance", "by value", vecs=std, topn=100)
        add("manhattan", "K=3 by value", vecs=std, topn=100)
        add("jaccard", "by row", rows=mrows, topn=100)
        add("anyof", "by row", rows=cat.any_rows, topn=100)
        add("bounded", "everything by value", vecs=std, metric="cosine", bound=-1.0, topn=10)
        add("diverse", "by value", vecs=std, lam=0.5, pool=pool, topn=10)
        add("capped", "by value, one per group", vecs=std, lam=1.0, pool=pool, mpg=1, topn=100)
        add("candidates", "descending list", vecs=std, metric="cosine", cand=cat.lists()["descending"], topn=100)
        add("scores", "descending list", vecs=std, metric="euclidean", cand=cat.lists()["descending"], topn=1)
        add("labels1", "by row", qrow=mrows[0], wanted=[L_ALL, L_ONE], topn=100)
        return [expect(cat, c) for c in out]

    # cosine playlist request
    for t in TOPNS:
        add("cosine", "plain by value", vecs=std, topn=t)
        add("cosine", "plain by row", rows=mrows, topn=t)
    wts = [1.0, -0.5, 0.75]
    add("cosine", "signed weights by value", vecs=std, weights=wts, topn=10)
    add("cosine", "signed weights by row", rows=mrows, weights=wts[:len(mrows)], topn=100)
    add("cosine", "band filter by row", rows=mrows, where=BAND, topn=10)
    add("cosine", "FEW filter by value", vecs=std, where=FEW, topn=100)
    add("cosine", "label of one shard", vecs=std, wanted=[L_ONE], topn=10)
    add("cosine", "label absent from a shard, by row", rows=mrows, wanted=[L_ABSENT], topn=100)
    add("cosine", "the common label", vecs=std, wanted=[L_ALL], topn=1024)
    add("cosine", "the two rare labels", vecs=std, wanted=[L_ONE, L_ABSENT], topn=100)
    add("cosine", "every label", vecs=std, wanted=[L_ONE, L_ALL, L_ABSENT], topn=10)
    add("cosine", "prior by value", vecs=std, prior=0.5, topn=10)
    add("cosine", "negative prior by row", rows=mrows, prior=-2.0, topn=100)
    add("cosine", "prior and label", vecs=std, prior=1.0, wanted=[L_ALL], topn=1)
    add("cosine", "scales by value", vecs=std, scales=SCALES, topn=10)
    add("cosine", "scales by row", rows=mrows, scales=SCALES, topn=1024)
    add("cosine", "seen= by row", rows=mrows, rowset=(cat.seen, "seen"), topn=10)
    add("cosine", "only= by value", vecs=std, rowset=(cat.only, "only"), topn=100)
    add("cosine", "only= and FEW", vecs=std, rowset=(cat.only, "only"), where=FEW, topn=1024)
    add("cosine", "exclusions over several shards by value", vecs=std, exclude=cat.several, topn=10)
    add("cosine", "exclusions over several shards by row", rows=mrows, exclude=cat.several, topn=100)
    add("cosine", f"{len(cat.k32)} members by row, 1024 excluded ids", rows=cat.k32, exclude=cat.x1024, topn=100)
    # distance request, distance scaled
    for t in TOPNS:
        add("distance", "by value", vecs=std, topn=t)
    add("distance", "by row", rows=mrows, topn=10)
    add("distance", "ids only (no distance pointer)", vecs=std, ids_only=True, topn=10)
    add("distance", "scaled by value", vecs=std, scales=SCALES, topn=10)
    add("distance", "scaled by row", rows=mrows, scales=SCALES, topn=100)
    add("distance", "seen=", vecs=std, rowset=(cat.seen, "seen"), topn=100)
    add("distance", "FEW filter", vecs=std, where=FEW, topn=100)
    add("distance", "exclusions over several shards", vecs=std, exclude=cat.several, topn=1024)
    # Manhattan: K = 1, 10 (the cut's last) and 11 (the first exact one)
    for k, t in ((1, 10), (10, 100), (11, 1024)):
        add("manhattan", f"K={k} by value", vecs=cat.l1_vecs[:k], topn=t)
    add("manhattan", "K=1 by row", rows=mrows[:1], topn=1)
    add("manhattan", "K=10 FEW filter", vecs=cat.l1_vecs[:10], where=FEW, topn=100)
    add("manhattan", "K=11 ids only", vecs=cat.l1_vecs, ids_only=True, topn=10)
    add("manhattan", "K=3 only=", vecs=std, rowset=(cat.only, "only"), topn=100)
    # Jaccard
    add("jaccard", "by value", vecs=std, topn=10)
    add("jaccard", "by value", vecs=std, topn=1024)
    add("jaccard", "by row", rows=mrows, topn=100)
    add("jaccard", "FEW filter", vecs=std, where=FEW, topn=100)
    add("jaccard", "by row", rows=mrows, topn=1)
    # any-of, always with out_member
    for t in TOPNS:
        add("anyof", "by value, a tie between members", vecs=cat.any_vecs, topn=t)
    add("anyof", "by row", rows=cat.any_rows, topn=10)
    add("anyof", "by row", rows=cat.any_rows, topn=100)
    add("anyof", "FEW filter", vecs=cat.any_vecs, where=FEW, topn=100)
    add("anyof", "only=", vecs=cat.any_vecs, rowset=(cat.only, "only"), topn=10)
    add("anyof", "label absent from a shard", vecs=cat.any_vecs, wanted=[L_ABSENT], topn=100)
    add("anyof", "without out_member (the plain merge)", vecs=cat.any_vecs, no_member=True, topn=100)
    # bounded: floor and radius; the bounds of bounded_oracle.bounds_for, and the floor at the short shard's worst row
    if "bounded" in kinds:
        for metric in ("cosine", "euclidean"):
            code = bounded_oracle.EUCLIDEAN if metric == "euclidean" else bounded_oracle.COSINE
            probe = expect(cat, Case("bounded", "", vecs=std, metric=metric, bound=0.0, topn=0))
            v = cat.cache[("bnd", _mkey(probe), code)]
            okb = bounded_oracle.admissible(cat.feats, v, [])
            floors = list(bounded_oracle.bounds_for(v, okb, code))
            for i, b in enumerate(floors):
                for t in (0, 10, 1024):
                    add("bounded", f"{metric} bound {b!r} by value", vecs=std, metric=metric, bound=b, topn=t)
                add("bounded", f"{metric} bound {b!r} by row", rows=mrows, metric=metric, bound=b, topn=(10, 1024, 0)[i % 3])
            if cat.short is not None and cat.sizes[cat.short] >= 3:           # a floor (a radius) that the short shard alone meets
                lo, hi = cat.bounds[cat.short]
                own = [r for r in range(lo + 1, min(hi, lo + 9)) if cat.feats[r, 11] == F32(0.25)]   # (not its neighbour's copy, not a FEW row)
                with np.errstate(all="ignore"):
                    b = float(v[own].min()) if metric == "cosine" else float(np.nextafter(np.sqrt(F32(0) - v[own].min()), F32(9)))
                for t in (0, 10, 1024):
                    add("bounded", f"{metric} bound {b!r}, the short shard's", vecs=std, metric=metric, bound=b, exclude=cat.hostile or None, topn=t)
            add("bounded", f"{metric} FEW filter", vecs=std, metric=metric, bound=floors[0], where=FEW, topn=100)
            add("bounded", f"{metric} seen=", vecs=std, metric=metric, bound=floors[0], rowset=(cat.seen, "seen"), topn=10)
    # diversified: the pool is larger than a shard's rows, and than n where 1024 allows
    for t, lam in ((1, 0.5), (10, 0.5), (10, 1.0), (100, 0.3), (1024, 0.7)):
        add("diverse", f"by value lambda {lam} pool {max(pool, t)}", vecs=std, lam=lam, pool=max(pool, t), topn=t)
    add("diverse", f"by row pool {pool}", rows=mrows, lam=0.5, pool=pool, topn=10)
    add("diverse", f"FEW filter pool {pool}", vecs=std, where=FEW, lam=0.5, pool=pool, topn=10)
    add("diverse", "exclusions over several shards, weights", vecs=std, weights=wts, exclude=cat.several, lam=0.0, pool=max(pool, 100), topn=100)
    # capped: group 0 has a row on every shard
    for mpg in (1, 2):
        for lam in (1.0, 0.7):
            add("capped", f"by value cap {mpg} lambda {lam}", vecs=std, lam=lam, pool=pool, mpg=mpg, topn=10)
            add("capped", f"by row cap {mpg} lambda {lam}", rows=mrows, lam=lam, pool=max(pool, 100), mpg=mpg, topn=100)
    add("capped", "FEW filter cap 1", vecs=std, where=FEW, lam=1.0, pool=pool, mpg=1, topn=10)
    # candidate lists and candidate scores
    for name, ids in cat.lists().items():
        add("candidates", f"cosine, list '{name}'", vecs=std, metric="cosine", cand=ids, topn=10)
        add("candidates", f"distance by row, list '{name}'", rows=mrows, metric="euclidean", cand=ids, topn=100)
        add("scores", f"cosine, list '{name}'", vecs=std, metric="cosine", cand=ids, topn=1)
        add("scores", f"distance by row, list '{name}'", rows=mrows, metric="euclidean", cand=ids, topn=1)
    every = cat.lists()["everything"]
    add("candidates", "cosine, everything, seen=, prior", vecs=std, metric="cosine", cand=every, rowset=(cat.seen, "seen"), prior=0.5, topn=1024)
    add("candidates", "distance, everything, FEW filter", vecs=std, metric="euclidean", cand=every, where=FEW, topn=1)
    add("scores", "cosine, everything, excluded and filtered rows", rows=mrows, metric="cosine", cand=every, exclude=cat.several, where=BAND, topn=1)
    add("scores", "distance, duplicates, excluded, label set", vecs=std, metric="euclidean", cand=cat.lists()["duplicates"], exclude=[0],
        wanted=[L_ALL], topn=1)
    # label-filtered single query
    for t in (10, 1024):
        add("labels1", "by row, label of one shard", qrow=mrows[0], wanted=[L_ONE], topn=t)
        add("labels1", "by value, label of one shard", qvec=std[0], qexcl=-1, wanted=[L_ONE], topn=t)
    add("labels1", "by row, a label no row has", qrow=mrows[0], wanted=[L_NONE], topn=10)
    add("labels1", "by value, a label no row has", qvec=std[0], qexcl=0, wanted=[L_NONE], topn=10)
    add("labels1", "by row, every label", qrow=mrows[-1], wanted=[L_ONE, L_ALL, L_ABSENT], topn=100)
    add("labels1", "by value, the two rare labels, a row excluded", qvec=std[1], qexcl=int(cat.bounds[cat.nonempty[0]][0]),
        wanted=[L_ONE, L_ABSENT], topn=100)
    return [expect(cat, c) for c in out]


@functools.lru_cache(maxsize=None)
def matrix(n: int, g: int, variant: str = "tied"):
    """The request matrix of a catalogue, made once per process (the expectations are never modified)."""
    return tuple(request_matrix(catalogue(n, g, variant), WIDE_KINDS if (n, g) == WIDE else KINDS))


def foreign_exclusions(cat):
    """An exclusion list with ids >= n (and rows of several shards): the single handle lets them match nothing, a node refuses."""
    return cat.several + [cat.n, cat.n + 7, 4_000_000_000]


def rowset_shapes(cat):
    """{name: ids}: the shapes of tests/test_gpu_rowset.py, exactly one shard, and everything but one shard."""
    from tests import rowset_oracle
    shapes = rowset_oracle.shapes(cat.n, SEED)
    mid = cat.nonempty[len(cat.nonempty) // 2]
    lo, hi = cat.bounds[mid]
    out = {k: shapes[k].tolist() for k in ("even", "low_nibble", "random30", "last_only")}
    out["one shard"] = list(range(lo, hi))
    out["all but one shard"] = [r for r in range(cat.n) if not lo <= r < hi]
    return out


def embed_requests(cat, d):
    """Request kwargs of EmbeddingTable.query for a geometry (tests/embed_cases.check takes them): by user vector and by member
    rows of different shards, the audio row on a one-row shard where there is one, topn above a shard's rows, exclusions over
    several shards."""
    rng = np.random.default_rng([SEED, cat.n, d])
    user = rng.standard_normal(d, dtype=F32)
    ones = [s for s in cat.nonempty if cat.sizes[s] == 1]
    audio_row = int(cat.bounds[ones[-1] if ones else cat.nonempty[-1]][0])
    top = min(1024, max(cat.sizes) + 3)
    edge_rows = [int(cat.bounds[s][0]) for s in cat.nonempty[:4]]
    return [dict(user=user, metric="cosine", embed_weight=1.0, topn=top),
            dict(rows=edge_rows, metric="cosine", embed_weight=0.25, audio_weight=1.0, audio_row=audio_row, topn=top, exclude=cat.several),
            dict(rows=edge_rows[::-1], metric="dot", embed_weight=-0.5, audio_weight=0.5, audio_row=audio_row, topn=10),
            dict(user=user, metric="dot", embed_weight=2.0, topn=1, exclude=cat.several)]


# ---- what the CPU leg asserts about the matrix, from the oracles' answers alone -----------------------------------------------
def spans_shards(cat, c) -> bool:
    return np.unique(cat.shard[c.ids]).size >= 2


def takes_a_whole_shard(cat, c) -> bool:
    """The short-list condition: some shard has admissible rows and the answer holds every one of them."""
    if c.ids.size == 0:
        return False
    taken = np.zeros(cat.n, bool)
    taken[c.ids] = True
    return any(c.adm[lo:hi].any() and taken[lo:hi][c.adm[lo:hi]].all() for lo, hi in cat.bounds if hi > lo)


def tied_pairs_in_order(cat, c) -> bool:
    """Every tied edge pair whose two rows are admissible comes with the lower id first (and, in an answer that is a top-N of
    one ranking, never the higher id without the lower)."""
    if c.kind == "scores" or c.get("prior") is not None:                      # (a prior differs between the two rows of a pair)
        return True
    pos = {int(r): i for i, r in enumerate(c.ids.tolist())}
    ranked = c.kind not in ("diverse", "capped")
    for a, b in cat.pairs:
        if not (c.adm[a] and c.adm[b]):
            continue
        if b in pos and (a in pos) and pos[a] > pos[b]:
            return False
        if ranked and b in pos and a not in pos:
            return False
    return True


def empty_share(catalogues=CATALOGUES):
    cases = [c for n, g, v in catalogues for c in matrix(n, g, v)]
    return sum(int(c.empty) for c in cases), len(cases)
