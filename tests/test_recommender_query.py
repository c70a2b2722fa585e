"""Recommender::Query / recommendQuery (include/Recommender.h) through csrc/shim_capi.cpp, on the 600-song catalogue of
tests/test_playlist_cpu.py::_write_csv (37 artists, 5 genres):

- re-initialisation: after a second initialize() on one object the new engine is handed the priors, groups and genres again
  on first use, and the class holds no row set (the set belonged to the engine that is gone).  On the CPU backend and, the same
  body, on the GPU.  Before the one-path refactor the second prior-weighted call failed on the CPU backend with "this handle
  has no priors (mi355rec_sharded_set_priors)" and the old set was still attached;
- the general recommendForPlaylist overload, recommendScaled and recommendNearest against the Query each of them fills;
- two faults in one call: the message printed is the one the commit before the refactor printed first (recorded there, through
  the overloads that existed: the general recommendForPlaylist and recommendScaled), asserted through those overloads and
  through recommendQuery."""
import ctypes

import numpy as np
import pytest


def _gpu_visible():
    from spotify_recommender_amd import capi
    return capi.lib().mi355rec_device_count() > 0


cpu_only = pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the CPU backend is never taken here")


class Shim:
    """One Recommender over a songs_data.bin (initialize(songs): genre ids and artist groups come from the songs)."""

    def __init__(self, path):
        from spotify_recommender_amd import build
        build.build_shim()
        L = self.L = ctypes.CDLL(str(build.LIB_SHIM))
        P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.shim_load.restype = P
        L.shim_load.argtypes = [ctypes.c_char_p]
        for name in ("shim_free", "shim_initialize", "shim_get_song_count"):
            getattr(L, name).argtypes = [P]
        L.shim_set_priors.argtypes = [P, P]
        L.shim_set_row_set.argtypes = [P, P, I, I]
        L.shim_artist_groups.argtypes = [P, P]
        L.shim_song_features.argtypes = [P, ctypes.c_int64, P, ctypes.POINTER(I)]
        L.shim_query.restype = ctypes.c_int64
        L.shim_query.argtypes = [P, P, I, P, I, P, P, P, I, P, I, P, I, I, F, I, I, F, P, I, I, I, P, P, ctypes.c_int64]
        L.shim_recommend_for_playlist.restype = L.shim_recommend_for_playlist_where.restype = ctypes.c_int64
        L.shim_recommend_for_playlist_weighted.restype = ctypes.c_int64
        L.shim_recommend_for_playlist.argtypes = [P, P, I, I, P, I, P, P, ctypes.c_int64]
        L.shim_recommend_for_playlist_where.argtypes = [P, P, I, I, P, P, P, I, P, I, P, P, ctypes.c_int64]
        L.shim_recommend_for_playlist_weighted.argtypes = [P, P, I, P, I, I, P, P, P, I, P, I, P, P, ctypes.c_int64]
        L.shim_recommend_for_playlist_general.restype = L.shim_recommend_scaled.restype = ctypes.c_int64
        L.shim_recommend_for_playlist_general.argtypes = [P, P, I, P, I, I, P, P, P, I, P, I, F, I, I, P, I, F, P, P, ctypes.c_int64]
        L.shim_recommend_scaled.argtypes = [P, P, I, I, P, I, I, P, P, P, I, P, I, P, P, ctypes.c_int64]
        self.h = L.shim_load(str(path).encode())
        assert self.h
        self.out, self.sc = np.full(1024, -7, np.int32), np.zeros(1024, np.float32)

    def close(self):
        self.L.shim_free(self.h)

    def initialize(self):
        assert self.L.shim_initialize(self.h) == 1
        self.n = self.L.shim_get_song_count(self.h)

    def set_priors(self, priors):
        p = np.ascontiguousarray(priors, np.float32)
        assert self.L.shim_set_priors(self.h, p.ctypes.data) == 1

    def set_rows(self, rows, only=False):
        a = np.asarray(rows, np.int32)
        assert self.L.shim_set_row_set(self.h, a.ctypes.data, len(rows), int(only)) == 1

    def groups_and_genres(self):
        g, f, genre = np.zeros(self.n, np.int32), np.zeros(12, np.float32), ctypes.c_int(0)
        self.L.shim_artist_groups(self.h, g.ctypes.data)
        genres = []
        for i in range(self.n):
            self.L.shim_song_features(self.h, i, f.ctypes.data, ctypes.byref(genre))
            genres.append(genre.value)
        return g, np.asarray(genres)

    def query(self, songs, topn, weights=(), where=(), exclude=(), genres=(), diverse=False, lam=1.0, pool=0, max_per_artist=0,
              prior_weight=0.0, scales=(), euclidean=False):
        """recommendQuery: (ids, score bits)."""
        s, w, ex, g, sca = _i32(songs), _f32(weights), _i32(exclude), _i32(genres), _f32(scales)
        wf, lo, hi = _i32(r[0] for r in where), _f32(r[1] for r in where), _f32(r[2] for r in where)
        n = self.L.shim_query(self.h, s.ctypes.data, len(songs), w.ctypes.data, len(weights), wf.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                              len(where), ex.ctypes.data, len(exclude), g.ctypes.data, len(genres), int(diverse), lam, pool, max_per_artist,
                              prior_weight, sca.ctypes.data, len(scales), int(euclidean), topn, self.out.ctypes.data, self.sc.ctypes.data, 1024)
        return self.out[:n].tolist(), self.sc[:n].view(np.uint32).tolist()


    def general(self, songs, topn, weights=(), where=(), exclude=(), lam=1.0, pool=0, max_per_artist=0, genres=(), prior_weight=0.0):
        """The most general recommendForPlaylist overload: (ids, score bits)."""
        s, w, ex, g = _i32(songs), _f32(weights), _i32(exclude), _i32(genres)
        wf, lo, hi = _i32(r[0] for r in where), _f32(r[1] for r in where), _f32(r[2] for r in where)
        n = self.L.shim_recommend_for_playlist_general(self.h, s.ctypes.data, len(songs), w.ctypes.data, len(weights), topn, wf.ctypes.data,
                                                       lo.ctypes.data, hi.ctypes.data, len(where), ex.ctypes.data, len(exclude), lam, pool,
                                                       max_per_artist, g.ctypes.data, len(genres), prior_weight, self.out.ctypes.data,
                                                       self.sc.ctypes.data, 1024)
        return self.out[:n].tolist(), self.sc[:n].view(np.uint32).tolist()

    def scaled(self, songs, topn, scales=(), euclidean=False, where=(), genres=()):
        """recommendScaled (euclidean without scales: recommendNearest): (ids, score bits)."""
        s, sca, g = _i32(songs), _f32(scales), _i32(genres)
        wf, lo, hi = _i32(r[0] for r in where), _f32(r[1] for r in where), _f32(r[2] for r in where)
        n = self.L.shim_recommend_scaled(self.h, s.ctypes.data, len(songs), topn, sca.ctypes.data, len(scales), int(euclidean), wf.ctypes.data,
                                         lo.ctypes.data, hi.ctypes.data, len(where), g.ctypes.data, len(genres), self.out.ctypes.data,
                                         self.sc.ctypes.data, 1024)
        return self.out[:n].tolist(), self.sc[:n].view(np.uint32).tolist()


def _i32(v):
    return np.asarray(list(v) or [0], np.int32)


def _f32(v):
    return np.asarray(list(v) or [0], np.float32)


@pytest.fixture(scope="module")
def songs_bin(tmp_path_factory):
    from spotify_recommender_amd import build
    from tests.test_playlist_cpu import _write_csv
    build.build_shim()
    d = tmp_path_factory.mktemp("query")
    _write_csv(d / "songs.csv")
    L = ctypes.CDLL(str(build.LIB_SHIM))
    L.shim_preprocess.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    assert L.shim_preprocess(str(d / "songs.csv").encode(), str(d / "songs_data.bin").encode()) == 1
    return d / "songs_data.bin"


MEMBERS = [5, 70]
PRIORS = [((i * 37) % 101) / 100 for i in range(600)]


def _reinitialisation(path):
    one, fresh = Shim(path), Shim(path)
    try:
        fresh.initialize()
        fresh.set_priors(PRIORS)
        want = fresh.query(MEMBERS, 8, prior_weight=0.5)
        assert len(want[0]) == 8
        one.initialize()
        one.set_priors(PRIORS)
        one.set_rows(want[0][:3])
        first = one.query(MEMBERS, 8, prior_weight=0.5)
        assert first[0][:5] == want[0][3:] and not set(first[0]) & set(want[0][:3])       # the set is applied
        one.initialize()                                                                  # ... and gone with its engine
        assert one.query(MEMBERS, 8, prior_weight=0.5) == want
        groups, genres = one.groups_and_genres()
        capped = one.query(MEMBERS, 8, max_per_artist=1)
        assert capped == fresh.query(MEMBERS, 8, max_per_artist=1) and len(capped[0]) == 8
        assert len(set(groups[capped[0]].tolist())) == 8                                  # one per artist
        within = one.query(MEMBERS, 8, genres=[2])
        assert within == fresh.query(MEMBERS, 8, genres=[2]) and len(within[0]) == 8 and set(genres[within[0]].tolist()) == {2}
        plain = fresh.query(MEMBERS, 8)
        gone = [plain[0][0], plain[0][4], 599]
        one.set_rows(gone)
        got = one.query(MEMBERS, 8)
        assert got == fresh.query(MEMBERS, 8, exclude=gone) and not set(got[0]) & set(gone)   # exactly its rows
        rest = [i for i in plain[0] if i not in gone]
        assert got[0][:len(rest)] == rest
    finally:
        one.close()
        fresh.close()


@cpu_only
def test_reinitialisation_on_the_cpu_backend(engine_lib, songs_bin):
    _reinitialisation(songs_bin)


@pytest.mark.gpu
def test_reinitialisation_on_the_gpu(engine_lib, songs_bin):
    import torch  # one HIP runtime per process: torch's first (see capi.lib)
    assert torch.cuda.is_available()
    _reinitialisation(songs_bin)


@cpu_only
def test_query_is_what_the_overloads_ask(engine_lib, songs_bin):
    """A Query filled by hand gives what the overload with the same arguments gives (here: the plain, the filtered and the
    weighted recommendForPlaylist)."""
    shim = Shim(songs_bin)
    try:
        shim.initialize()
        L, out, sc = shim.L, np.full(1024, -7, np.int32), np.zeros(1024, np.float32)
        s, ex = np.asarray(MEMBERS, np.int32), np.asarray([3, 9], np.int32)
        n = L.shim_recommend_for_playlist(shim.h, s.ctypes.data, 2, 10, ex.ctypes.data, 2, out.ctypes.data, sc.ctypes.data, 1024)
        assert (out[:n].tolist(), sc[:n].view(np.uint32).tolist()) == shim.query(MEMBERS, 10, exclude=[3, 9])
        f, lo, hi = np.asarray([1], np.int32), np.asarray([0.2], np.float32), np.asarray([0.9], np.float32)
        n = L.shim_recommend_for_playlist_where(shim.h, s.ctypes.data, 2, 10, f.ctypes.data, lo.ctypes.data, hi.ctypes.data, 1, ex.ctypes.data, 0,
                                                out.ctypes.data, sc.ctypes.data, 1024)
        assert (out[:n].tolist(), sc[:n].view(np.uint32).tolist()) == shim.query(MEMBERS, 10, where=[(1, 0.2, 0.9)])
        w = np.asarray([1.0, -0.5], np.float32)
        n = L.shim_recommend_for_playlist_weighted(shim.h, s.ctypes.data, 2, w.ctypes.data, 2, 10, f.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                                   0, ex.ctypes.data, 0, out.ctypes.data, sc.ctypes.data, 1024)
        assert (out[:n].tolist(), sc[:n].view(np.uint32).tolist()) == shim.query(MEMBERS, 10, weights=[1.0, -0.5])
    finally:
        shim.close()


@cpu_only
def test_the_general_overload_and_recommend_scaled_are_their_queries(engine_lib, songs_bin, capfd):
    """The overloads whose bodies became a few lines that fill a Query: the same ids and score bits as that Query, for the
    branches of the general overload (maxPerArtist 0 within genres or with a prior weight: no cap; lambda 1 then: the plain
    request; maxPerArtist 0 without either: refused) and for recommendScaled / recommendNearest under either metric."""
    shim = Shim(songs_bin)
    try:
        shim.initialize()
        shim.set_priors(PRIORS)
        _, genres = shim.groups_and_genres()
        where, scales = [(1, 0.2, 0.9)], [1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 0.5, 1.0]
        plain = shim.query(MEMBERS, 10, genres=[1, 2])
        assert len(plain[0]) == 10 and set(genres[plain[0]].tolist()) <= {1, 2}
        assert shim.general(MEMBERS, 10, genres=[1, 2]) == plain                                             # lambda 1, no cap: the plain request
        assert shim.query(MEMBERS, 10, genres=[1, 2], diverse=True) == plain
        spread = shim.general(MEMBERS, 10, lam=0.3, genres=[1, 2])                                           # maxPerArtist 0: no cap
        assert spread == shim.query(MEMBERS, 10, genres=[1, 2], diverse=True, lam=0.3) and spread != plain
        capped = shim.general(MEMBERS, 10, weights=[1.0, -0.5], where=where, exclude=[3], lam=0.7, pool=64, max_per_artist=1, genres=[1, 2],
                              prior_weight=0.5)
        assert capped == shim.query(MEMBERS, 10, weights=[1.0, -0.5], where=where, exclude=[3], diverse=True, lam=0.7, pool=64,
                                    max_per_artist=1, genres=[1, 2], prior_weight=0.5) and len(capped[0]) == 10
        assert shim.general(MEMBERS, 10, prior_weight=-1.0) == shim.query(MEMBERS, 10, prior_weight=-1.0) != shim.query(MEMBERS, 10)
        assert shim.general(MEMBERS, 10, max_per_artist=2) == shim.query(MEMBERS, 10, max_per_artist=2)
        capfd.readouterr()
        assert shim.general(MEMBERS, 10) == ([], [])                                                         # maxPerArtist 0 and nothing else
        assert capfd.readouterr().err == "Error: maxPerArtist must be positive\n"
        cosine = shim.scaled(MEMBERS, 10, scales, where=where, genres=[1, 2])
        nearest = shim.scaled(MEMBERS, 10, scales, euclidean=True, where=where, genres=[1, 2])
        assert cosine == shim.query(MEMBERS, 10, scales=scales, where=where, genres=[1, 2]) and len(cosine[0]) == 10
        assert nearest == shim.query(MEMBERS, 10, scales=scales, euclidean=True, where=where, genres=[1, 2]) and len(nearest[0]) == 10
        assert nearest != cosine and cosine != shim.query(MEMBERS, 10, where=where, genres=[1, 2])
        assert shim.scaled(MEMBERS, 10) == shim.query(MEMBERS, 10)
        assert shim.scaled(MEMBERS, 10, euclidean=True) == shim.query(MEMBERS, 10, euclidean=True) != shim.query(MEMBERS, 10)
        dist = np.asarray(shim.scaled(MEMBERS, 10, euclidean=True)[1], np.uint32).view(np.float32)
        assert (np.diff(dist) >= 0).all() and dist[0] > 0                                                    # distances, nearest first
    finally:
        shim.close()


# what the overloads of the commit before the refactor printed for a call with two faults (stderr, whole), through the overloads
OVERLOAD_TWO_FAULTS = [
    ("general:weights+index", "general", dict(songs=[9999], topn=5, weights=[1.0, 2.0], genres=[1]),
     "Error: 2 weights for 1 songs (one weight per song, or none)\n"),
    ("general:range+empty", "general", dict(songs=[], topn=5, where=[(1, 0.9, 0.2)], genres=[1]),
     "Error: invalid range [0.9, 0.2] on feature 1\n"),
    ("general:excluded+index", "general", dict(songs=[9999], topn=5, exclude=[3] * 1025, genres=[1]),
     "Error: at most 1024 songs can be excluded\n"),
    ("general:cap0+index", "general", dict(songs=[9999], topn=5), "Error: Invalid song index: 9999\n"),
    ("general:cap-1+pool-2", "general", dict(songs=[1], topn=5, lam=0.5, pool=-2, max_per_artist=-1, genres=[1]),
     "Error: pool must be positive (or 0 for the default)\n"),
    ("scaled:range+empty", "scaled", dict(songs=[], topn=5, where=[(1, 0.9, 0.2)]), "Error: a playlist holds 1 to 32 songs\n"),
    ("scaled:range+scales", "scaled", dict(songs=[1], topn=5, scales=[1.0, 2.0, 3.0], where=[(1, 0.9, 0.2)]),
     "Error: 3 feature scales: one per feature, 12 in all\n"),
    ("scaled:range+index", "scaled", dict(songs=[9999], topn=5, euclidean=True, scales=[1.0] * 12, where=[(1, 0.9, 0.2)]),
     "Error: Invalid song index: 9999\n"),
    ("scaled:scales+topn", "scaled", dict(songs=[1], topn=0, scales=[1.0, 2.0, 3.0]), "Error: topN must be positive\n"),
    ("nearest:range+topn", "scaled", dict(songs=[1], topn=0, euclidean=True, where=[(1, 0.9, 0.2)]), "Error: topN must be positive\n"),
    ("scaled:range", "scaled", dict(songs=[1], topn=5, where=[(1, 0.9, 0.2)]), "Error: invalid range [0.9, 0.2] on feature 1\n"),
]


@cpu_only
@pytest.mark.parametrize("name,method,call,said", OVERLOAD_TWO_FAULTS, ids=[t[0] for t in OVERLOAD_TWO_FAULTS])
def test_the_overloads_report_the_fault_they_reported_before(engine_lib, songs_bin, capfd, name, method, call, said):
    shim = Shim(songs_bin)
    try:
        shim.initialize()
        capfd.readouterr()
        assert getattr(shim, method)(**call) == ([], [])
        assert capfd.readouterr().err == said
    finally:
        shim.close()


# what the commit before the refactor printed for a call with two faults (stderr, whole)
TWO_FAULTS = [
    ("weights+index", dict(songs=[9999], topn=5, weights=[1.0, 2.0], genres=[1]),
     "Error: 2 weights for 1 songs (one weight per song, or none)\n"),
    ("range+empty", dict(songs=[], topn=5, where=[(1, 0.9, 0.2)], genres=[1]),
     "Error: invalid range [0.9, 0.2] on feature 1\n"),
    ("scales+topn", dict(songs=[1], topn=0, scales=[1.0, 2.0, 3.0]),
     "Error: topN must be positive\n"),
    ("excluded+index", dict(songs=[9999], topn=5, exclude=[3] * 1025, genres=[1]),
     "Error: at most 1024 songs can be excluded\n"),
]


@cpu_only
@pytest.mark.parametrize("name,call,said", TWO_FAULTS, ids=[t[0] for t in TWO_FAULTS])
def test_the_first_of_two_faults_is_the_one_reported_before(engine_lib, songs_bin, capfd, name, call, said):
    shim = Shim(songs_bin)
    try:
        shim.initialize()
        capfd.readouterr()
        assert shim.query(**call) == ([], [])
        assert capfd.readouterr().err == said
    finally:
        shim.close()


@cpu_only
def test_each_fault_alone_has_its_message(engine_lib, songs_bin, capfd):
    """The second fault of each pair above, alone: the pairs test an order, not one check that hides another for good."""
    shim = Shim(songs_bin)
    try:
        shim.initialize()
        for call, said in ((dict(songs=[9999], topn=5), "Error: Invalid song index: 9999\n"),
                           (dict(songs=[], topn=5), "Error: a playlist holds 1 to 32 songs\n"),
                           (dict(songs=[1], topn=5, scales=[1.0, 2.0, 3.0]), "Error: 3 feature scales: one per feature, 12 in all\n"),
                           (dict(songs=[1], topn=5, euclidean=True, weights=[1.0]),
                            "Error: the Euclidean metric takes no weights, diversity, cap or prior weight\n")):
            capfd.readouterr()
            assert shim.query(**call) == ([], [])
            assert capfd.readouterr().err == said
    finally:
        shim.close()
