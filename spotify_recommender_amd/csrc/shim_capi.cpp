// shim_capi.cpp — plain-C handles onto the C++ drop-in classes so that the
// parity tests (ctypes) can drive Recommender / DataManager exactly as
// main.cpp does.  Test/tooling surface only; applications use the classes.
#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "DataManager.h"
#include "Recommender.h"
#include "Song.h"

namespace {
struct Catalogue {
    std::vector<Song> songs;
    std::map<int, std::string> genres;
    Recommender rec;
};
int64_t copyOut(const std::string& s, char* out, int64_t cap) {
    const int64_t n = static_cast<int64_t>(s.size()) < cap ? static_cast<int64_t>(s.size()) : cap;
    if (n > 0) std::memcpy(out, s.data(), static_cast<size_t>(n));
    return static_cast<int64_t>(s.size());
}
}  // namespace

extern "C" {

int shim_preprocess(const char* csv, const char* out) { return DataManager::preprocessData(csv, out) ? 1 : 0; }

void* shim_load(const char* bin) {
    Catalogue* c = new Catalogue();
    if (!DataManager::loadData(bin, c->songs, c->genres)) {
        delete c;
        return nullptr;
    }
    return c;
}

void* shim_from_matrix(const float* feats, int64_t n) {
    Catalogue* c = new Catalogue();
    c->songs.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        c->songs[i].track_id = "id" + std::to_string(i);
        c->songs[i].track_name = "Song " + std::to_string(i);
        std::memcpy(c->songs[i].features, feats + i * FEATURE_COUNT, sizeof(float) * FEATURE_COUNT);
    }
    return c;
}

// The CLI's query-mode path: DataManager::loadCatalogue + the matrix overload of
// Recommender::initialize.  Songs are only materialised one at a time (readSong).
struct FastCatalogue {
    DataManager::Catalogue cat;
    Recommender rec;
};

void* shim_fast_load(const char* bin) {
    FastCatalogue* c = new FastCatalogue();
    if (!DataManager::loadCatalogue(bin, c->cat)) {
        delete c;
        return nullptr;
    }
    return c;
}
int shim_fast_initialize(void* h) {
    FastCatalogue* c = static_cast<FastCatalogue*>(h);
    return c->rec.initialize(c->cat.features, c->cat.trackIds, c->cat.trackNames) ? 1 : 0;
}
void shim_fast_free(void* h) { delete static_cast<FastCatalogue*>(h); }
int64_t shim_fast_song_count(void* h) { return static_cast<int64_t>(static_cast<FastCatalogue*>(h)->cat.size()); }
int64_t shim_fast_recommend(void* h, const char* id, int topn, int* out, int64_t cap) {
    FastCatalogue* c = static_cast<FastCatalogue*>(h);
    const std::vector<int> r = c->rec.recommend(id, topn);
    for (size_t i = 0; i < r.size() && static_cast<int64_t>(i) < cap; ++i) out[i] = r[i];
    return static_cast<int64_t>(r.size());
}
int64_t shim_fast_recommend_by_name(void* h, const char* name, int topn, int* out, int64_t cap) {
    FastCatalogue* c = static_cast<FastCatalogue*>(h);
    const std::vector<int> r = c->rec.recommendByName(name, topn);
    for (size_t i = 0; i < r.size() && static_cast<int64_t>(i) < cap; ++i) out[i] = r[i];
    return static_cast<int64_t>(r.size());
}
// which: 0 id, 1 name, 2 artists, 3 genre name — read back from the file through readSong
int64_t shim_fast_song_string(void* h, int64_t i, int which, char* out, int64_t cap) {
    FastCatalogue* c = static_cast<FastCatalogue*>(h);
    Song s;
    if (i < 0 || !DataManager::readSong(c->cat, static_cast<size_t>(i), s)) return -1;
    if (which == 3) return copyOut(c->cat.genreMap[s.genre_id], out, cap);
    return copyOut(which == 0 ? s.track_id : which == 1 ? s.track_name : s.artists, out, cap);
}
// writes a synthetic songs_data.bin (Song::serialize) straight from a feature matrix: test fixture
int shim_write_synthetic_bin(const char* path, const float* feats, int64_t n, int genres) {
    std::ofstream out(path, std::ios::binary);
    if (!out.is_open()) return 0;
    const size_t numSongs = static_cast<size_t>(n), numGenres = static_cast<size_t>(genres);
    out.write(reinterpret_cast<const char*>(&numSongs), sizeof numSongs);
    out.write(reinterpret_cast<const char*>(&numGenres), sizeof numGenres);
    for (int g = 0; g < genres; ++g) {
        const std::string name = "genre-" + std::to_string(g);
        const size_t len = name.size();
        out.write(reinterpret_cast<const char*>(&g), sizeof g);
        out.write(reinterpret_cast<const char*>(&len), sizeof len);
        out.write(name.data(), static_cast<std::streamsize>(len));
    }
    Song s;
    for (int64_t i = 0; i < n; ++i) {
        s.track_id = "id" + std::to_string(i);
        s.track_name = "Song " + std::to_string(i);
        s.artists = "Artist " + std::to_string(i % 977);
        s.genre_id = static_cast<int>(i % genres);
        std::memcpy(s.features, feats + i * FEATURE_COUNT, sizeof(float) * FEATURE_COUNT);
        s.serialize(out);
    }
    return out.good() ? 1 : 0;
}

void shim_free(void* h) { delete static_cast<Catalogue*>(h); }
int64_t shim_song_count(void* h) { return static_cast<int64_t>(static_cast<Catalogue*>(h)->songs.size()); }
int64_t shim_genre_count(void* h) { return static_cast<int64_t>(static_cast<Catalogue*>(h)->genres.size()); }

int shim_song_features(void* h, int64_t i, float* out12, int* genre) {
    Catalogue* c = static_cast<Catalogue*>(h);
    if (i < 0 || i >= static_cast<int64_t>(c->songs.size())) return 0;
    std::memcpy(out12, c->songs[i].features, sizeof(float) * FEATURE_COUNT);
    *genre = c->songs[i].genre_id;
    return 1;
}

int64_t shim_song_string(void* h, int64_t i, int which, char* out, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    if (i < 0 || i >= static_cast<int64_t>(c->songs.size())) return -1;
    const Song& s = c->songs[i];
    return copyOut(which == 0 ? s.track_id : which == 1 ? s.track_name : s.artists, out, cap);
}

int64_t shim_genre_name(void* h, int id, char* out, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    const auto it = c->genres.find(id);
    return it == c->genres.end() ? -1 : copyOut(it->second, out, cap);
}


int shim_initialize(void* h) { Catalogue* c = static_cast<Catalogue*>(h); return c->rec.initialize(c->songs) ? 1 : 0; }
int shim_is_initialized(void* h) { return static_cast<Catalogue*>(h)->rec.isInitialized() ? 1 : 0; }
int shim_is_gpu_enabled(void* h) { return static_cast<Catalogue*>(h)->rec.isGPUEnabled() ? 1 : 0; }
int shim_get_song_count(void* h) { return static_cast<Catalogue*>(h)->rec.getSongCount(); }

static int64_t giveBack(Catalogue* c, const std::vector<int>& r, int* out, float* scores, int64_t cap) {
    const int64_t n = static_cast<int64_t>(r.size()) < cap ? static_cast<int64_t>(r.size()) : cap;
    for (int64_t i = 0; i < n; ++i) {
        out[i] = r[i];
        if (scores) scores[i] = c->rec.lastScores()[i];
    }
    return static_cast<int64_t>(r.size());
}

int64_t shim_recommend_by_index(void* h, int idx, int topn, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendByIndex(idx, topn), out, scores, cap);
}
int64_t shim_recommend(void* h, const char* id, int topn, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommend(id, topn), out, scores, cap);
}
int64_t shim_recommend_by_name(void* h, const char* name, int topn, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendByName(name, topn), out, scores, cap);
}
// Recommender::recommendByIndexInGenres; genre_ids (one per song, may be null) goes to setGenreIds first.
int64_t shim_recommend_by_index_in_genres(void* h, int idx, int topn, const int* genres, int n_genres, const int* genre_ids,
                                          int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    if (genre_ids && !c->rec.setGenreIds(std::vector<int>(genre_ids, genre_ids + c->rec.getSongCount()))) return -1;
    return giveBack(c, c->rec.recommendByIndexInGenres(idx, topn, std::vector<int>(genres, genres + (n_genres > 0 ? n_genres : 0))),
                    out, scores, cap);
}
// Recommender::setRowSet (n_songs < 0: clearRowSet).
int shim_set_row_set(void* h, const int* songs, int n_songs, int only) {
    Catalogue* c = static_cast<Catalogue*>(h);
    if (n_songs < 0) {
        c->rec.clearRowSet();
        return 1;
    }
    return c->rec.setRowSet(std::vector<int>(songs, songs + n_songs), only != 0) ? 1 : 0;
}
// Recommender::setCandidates (n_songs < 0: clearCandidates).
int shim_set_candidates(void* h, const int64_t* songs, int64_t n_songs) {
    Catalogue* c = static_cast<Catalogue*>(h);
    if (n_songs < 0) {
        c->rec.clearCandidates();
        return 1;
    }
    return c->rec.setCandidates(std::vector<int64_t>(songs, songs + n_songs)) ? 1 : 0;
}
// Recommender::scoreSongs of the Query {songs, alsoExclude = exclude, where = the one range on where_feature (< 0: none), euclidean,
// diverse, maxPerArtist, topN}: the values and flags of the n_listed songs into values / admissible (either may be null); returns how
// many values the class gave back (0: refused, or an empty list).
int64_t shim_score_songs(void* h, const int* songs, int n_songs, const int* exclude, int n_exclude, int where_feature, float lo, float hi,
                         int euclidean, int diverse, int max_per_artist, int topn, const int64_t* listed, int64_t n_listed, float* values,
                         char* admissible) {
    Catalogue* c = static_cast<Catalogue*>(h);
    Recommender::Query q;
    q.songs.assign(songs, songs + (n_songs > 0 ? n_songs : 0));
    q.alsoExclude.assign(exclude, exclude + (n_exclude > 0 ? n_exclude : 0));
    if (where_feature >= 0) q.where.push_back({where_feature, lo, hi});
    q.euclidean = euclidean != 0;
    q.diverse = diverse != 0;
    q.lambda = 0.5f;
    q.maxPerArtist = max_per_artist;
    q.topN = topn;
    std::vector<char> flags;
    const std::vector<float> v = c->rec.scoreSongs(q, std::vector<int64_t>(listed, listed + (n_listed > 0 ? n_listed : 0)), &flags);
    for (size_t i = 0; i < v.size(); ++i) {
        if (values) values[i] = v[i];
        if (admissible) admissible[i] = flags[i];
    }
    return static_cast<int64_t>(v.size());
}
// Recommender::recommendQuery of the any-of Query {songs, alsoExclude = exclude, where = the one range on where_feature (< 0: none),
// topN, anyOf}, and — `refuse`, a bit each, to show the refusals — with weights (1), diverse (2), maxPerArtist (4), priorWeight (8),
// scales (16), euclidean (32), or through scoreSongs (64).  matched (may be null): lastMatchedSongs().  Returns how many songs came back.
int64_t shim_query_anyof(void* h, const int* songs, int n_songs, const int* exclude, int n_exclude, int where_feature, float lo, float hi,
                         int topn, int refuse, int* out, float* scores, int* matched, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    Recommender::Query q;
    q.songs.assign(songs, songs + (n_songs > 0 ? n_songs : 0));
    q.alsoExclude.assign(exclude, exclude + (n_exclude > 0 ? n_exclude : 0));
    if (where_feature >= 0) q.where.push_back({where_feature, lo, hi});
    q.topN = topn;
    q.anyOf = true;
    if (refuse & 1) q.weights.assign(q.songs.size(), 1.0f);
    if (refuse & 2) q.diverse = true, q.lambda = 0.5f;
    if (refuse & 4) q.maxPerArtist = 1;
    if (refuse & 8) q.priorWeight = 0.5f;
    if (refuse & 16) q.scales.assign(12, 2.0f);
    if (refuse & 32) q.euclidean = true;
    if (refuse & 64) return static_cast<int64_t>(c->rec.scoreSongs(q, std::vector<int64_t>{0}).size());
    const int64_t n = giveBack(c, c->rec.recommendQuery(q), out, scores, cap);
    const std::vector<int>& m = c->rec.lastMatchedSongs();
    for (int64_t i = 0; matched && i < n && i < cap && i < static_cast<int64_t>(m.size()); ++i) matched[i] = m[static_cast<size_t>(i)];
    return m.size() == static_cast<size_t>(n) ? n : -1;
}
// Recommender::recommendQuery of the Manhattan Query {songs, alsoExclude = exclude, where = the one range on where_feature (< 0:
// none), topN, manhattan}, and — `refuse`, a bit each, to show the refusals — with weights (1), diverse (2), maxPerArtist (4),
// priorWeight (8), scales (16), euclidean (32), through scoreSongs (64), anyOf (128) or with a candidate list set (256).  scores:
// lastScores(), the distances.  Returns how many songs came back.
int64_t shim_query_manhattan(void* h, const int* songs, int n_songs, const int* exclude, int n_exclude, int where_feature, float lo, float hi,
                             int topn, int refuse, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    Recommender::Query q;
    q.songs.assign(songs, songs + (n_songs > 0 ? n_songs : 0));
    q.alsoExclude.assign(exclude, exclude + (n_exclude > 0 ? n_exclude : 0));
    if (where_feature >= 0) q.where.push_back({where_feature, lo, hi});
    q.topN = topn;
    q.manhattan = true;
    if (refuse & 1) q.weights.assign(q.songs.size(), 1.0f);
    if (refuse & 2) q.diverse = true, q.lambda = 0.5f;
    if (refuse & 4) q.maxPerArtist = 1;
    if (refuse & 8) q.priorWeight = 0.5f;
    if (refuse & 16) q.scales.assign(12, 2.0f);
    if (refuse & 32) q.euclidean = true;
    if (refuse & 128) q.anyOf = true;
    if (refuse & 64) return static_cast<int64_t>(c->rec.scoreSongs(q, std::vector<int64_t>{0}).size());
    if (refuse & 256) c->rec.setCandidates(std::vector<int64_t>{0, 1, 2});
    const int64_t n = giveBack(c, c->rec.recommendQuery(q), out, scores, cap);
    if (refuse & 256) c->rec.clearCandidates();
    return n;
}
// Recommender::recommendQuery of the bounded Query {songs, alsoExclude = exclude, where = the one range on where_feature (< 0: none),
// topN}.atLeast(bound) or, with `euclidean`, .within(bound), and — `refuse`, a bit each, to show the refusals — with weights (1),
// diverse (2), maxPerArtist (4), priorWeight (8), scales (16), through scoreSongs (64), anyOf (128), with a candidate list set (256)
// or manhattan (512).  scores: lastScores().  *match_count: lastMatchCount().  Returns how many songs came back.
int64_t shim_query_bounded(void* h, const int* songs, int n_songs, const int* exclude, int n_exclude, int where_feature, float lo, float hi,
                           int topn, int euclidean, float bound, int refuse, int* out, float* scores, long long* match_count, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    Recommender::Query q;
    q.songs.assign(songs, songs + (n_songs > 0 ? n_songs : 0));
    q.alsoExclude.assign(exclude, exclude + (n_exclude > 0 ? n_exclude : 0));
    if (where_feature >= 0) q.where.push_back({where_feature, lo, hi});
    q.topN = topn;
    if (euclidean) q.within(bound);
    else q.atLeast(bound);
    if (refuse & 1) q.weights.assign(q.songs.size(), 1.0f);
    if (refuse & 2) q.diverse = true, q.lambda = 0.5f;
    if (refuse & 4) q.maxPerArtist = 1;
    if (refuse & 8) q.priorWeight = 0.5f;
    if (refuse & 16) q.scales.assign(12, 2.0f);
    if (refuse & 128) q.anyOf = true;
    if (refuse & 512) q.manhattan = true;
    if (refuse & 64) return static_cast<int64_t>(c->rec.scoreSongs(q, std::vector<int64_t>{0}).size());
    if (refuse & 256) c->rec.setCandidates(std::vector<int64_t>{0, 1, 2});
    const int64_t n = giveBack(c, c->rec.recommendQuery(q), out, scores, cap);
    if (refuse & 256) c->rec.clearCandidates();
    if (match_count) *match_count = c->rec.lastMatchCount();
    return n;
}
// Recommender::recommendQuery of the Jaccard Query {songs, alsoExclude = exclude, where = the one range on where_feature (< 0: none),
// topN, jaccard}, and — `refuse`, a bit each, to show the refusals — with weights (1), diverse (2), maxPerArtist (4), priorWeight (8),
// scales (16), euclidean (32), through scoreSongs (64), anyOf (128), with a candidate list set (256), manhattan (512) or a bound
// (1024).  scores: lastScores(), the similarities.  Returns how many songs came back.
int64_t shim_query_jaccard(void* h, const int* songs, int n_songs, const int* exclude, int n_exclude, int where_feature, float lo, float hi,
                           int topn, int refuse, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    Recommender::Query q;
    q.songs.assign(songs, songs + (n_songs > 0 ? n_songs : 0));
    q.alsoExclude.assign(exclude, exclude + (n_exclude > 0 ? n_exclude : 0));
    if (where_feature >= 0) q.where.push_back({where_feature, lo, hi});
    q.topN = topn;
    if (refuse & 1024) q.atLeast(0.5f);
    q.jaccard = true;
    if (refuse & 1) q.weights.assign(q.songs.size(), 1.0f);
    if (refuse & 2) q.diverse = true, q.lambda = 0.5f;
    if (refuse & 4) q.maxPerArtist = 1;
    if (refuse & 8) q.priorWeight = 0.5f;
    if (refuse & 16) q.scales.assign(12, 2.0f);
    if (refuse & 32) q.euclidean = true;
    if (refuse & 128) q.anyOf = true;
    if (refuse & 512) q.manhattan = true;
    if (refuse & 64) return static_cast<int64_t>(c->rec.scoreSongs(q, std::vector<int64_t>{0}).size());
    if (refuse & 256) c->rec.setCandidates(std::vector<int64_t>{0, 1, 2});
    const int64_t n = giveBack(c, c->rec.recommendQuery(q), out, scores, cap);
    if (refuse & 256) c->rec.clearCandidates();
    return n;
}
// Recommender::updateSongs (n_features floats for n_songs songs: a length that differs is refused by the class).
int shim_update_songs(void* h, const int* songs, int n_songs, const float* features, int64_t n_features) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return c->rec.updateSongs(std::vector<int>(songs, songs + (n_songs > 0 ? n_songs : 0)),
                              std::vector<float>(features, features + (n_features > 0 ? n_features : 0))) ? 1 : 0;
}
// Recommender::recommendForPlaylist.
int64_t shim_recommend_for_playlist(void* h, const int* songs, int n_songs, int topn, const int* exclude, int n_exclude, int* out,
                                    float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForPlaylist(std::vector<int>(songs, songs + (n_songs > 0 ? n_songs : 0)), topn,
                                                   std::vector<int>(exclude, exclude + (n_exclude > 0 ? n_exclude : 0))),
                    out, scores, cap);
}
// Recommender::recommendByIndexWhere and the filtered recommendForPlaylist: n_ranges ranges (features[i], lo[i], hi[i]).
static std::vector<Recommender::FeatureRange> ranges(const int* features, const float* lo, const float* hi, int n_ranges) {
    std::vector<Recommender::FeatureRange> r;
    for (int i = 0; i < n_ranges; ++i) r.push_back({features[i], lo[i], hi[i]});
    return r;
}
int64_t shim_recommend_by_index_where(void* h, int idx, int topn, const int* features, const float* lo, const float* hi, int n_ranges,
                                      int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendByIndexWhere(idx, topn, ranges(features, lo, hi, n_ranges)), out, scores, cap);
}
int64_t shim_recommend_for_playlist_where(void* h, const int* songs, int n_songs, int topn, const int* features, const float* lo,
                                          const float* hi, int n_ranges, const int* exclude, int n_exclude, int* out, float* scores,
                                          int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForPlaylist(std::vector<int>(songs, songs + (n_songs > 0 ? n_songs : 0)), topn,
                                                   ranges(features, lo, hi, n_ranges),
                                                   std::vector<int>(exclude, exclude + (n_exclude > 0 ? n_exclude : 0))),
                    out, scores, cap);
}
// The weighted recommendForPlaylist (n_weights weights for n_songs songs: a length that differs is refused by the class) and
// recommendForTaste.
int64_t shim_recommend_for_playlist_weighted(void* h, const int* songs, int n_songs, const float* weights, int n_weights, int topn,
                                             const int* features, const float* lo, const float* hi, int n_ranges, const int* exclude,
                                             int n_exclude, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForPlaylist(std::vector<int>(songs, songs + (n_songs > 0 ? n_songs : 0)), topn,
                                                   std::vector<float>(weights, weights + (n_weights > 0 ? n_weights : 0)),
                                                   ranges(features, lo, hi, n_ranges),
                                                   std::vector<int>(exclude, exclude + (n_exclude > 0 ? n_exclude : 0))),
                    out, scores, cap);
}
int64_t shim_recommend_for_taste(void* h, const int* liked, int n_liked, const int* disliked, int n_disliked, int topn,
                                 float dislike_weight, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForTaste(std::vector<int>(liked, liked + (n_liked > 0 ? n_liked : 0)),
                                                std::vector<int>(disliked, disliked + (n_disliked > 0 ? n_disliked : 0)), topn,
                                                dislike_weight),
                    out, scores, cap);
}
// recommendDiverse and the diversified recommendForPlaylist (n_weights 0: no weights).
int64_t shim_recommend_diverse(void* h, int song, int topn, float lambda, int pool, const int* features, const float* lo, const float* hi,
                               int n_ranges, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendDiverse(song, topn, lambda, pool, ranges(features, lo, hi, n_ranges)), out, scores, cap);
}
int64_t shim_recommend_for_playlist_diverse(void* h, const int* songs, int n_songs, const float* weights, int n_weights, int topn,
                                            const int* features, const float* lo, const float* hi, int n_ranges, const int* exclude,
                                            int n_exclude, float lambda, int pool, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForPlaylist(std::vector<int>(songs, songs + (n_songs > 0 ? n_songs : 0)), topn,
                                                   std::vector<float>(weights, weights + (n_weights > 0 ? n_weights : 0)),
                                                   ranges(features, lo, hi, n_ranges),
                                                   std::vector<int>(exclude, exclude + (n_exclude > 0 ? n_exclude : 0)), lambda, pool),
                    out, scores, cap);
}
// recommendByIndexCapped and the capped recommendForPlaylist; group_ids (one per song, may be null) goes to setGroupIds first,
// null keeps the groups initialize derived from the songs' artists.  shim_song_group: that derivation for song i.
int64_t shim_recommend_capped(void* h, int song, int topn, int max_per_artist, float lambda, int pool, const int* features, const float* lo,
                              const float* hi, int n_ranges, const int* group_ids, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    if (group_ids && !c->rec.setGroupIds(std::vector<int>(group_ids, group_ids + c->rec.getSongCount()))) return -1;
    return giveBack(c, c->rec.recommendByIndexCapped(song, topn, max_per_artist, lambda, pool, ranges(features, lo, hi, n_ranges)), out,
                    scores, cap);
}
int64_t shim_recommend_for_playlist_capped(void* h, const int* songs, int n_songs, const float* weights, int n_weights, int topn,
                                           const int* features, const float* lo, const float* hi, int n_ranges, const int* exclude,
                                           int n_exclude, float lambda, int pool, int max_per_artist, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForPlaylist(std::vector<int>(songs, songs + (n_songs > 0 ? n_songs : 0)), topn,
                                                   std::vector<float>(weights, weights + (n_weights > 0 ? n_weights : 0)),
                                                   ranges(features, lo, hi, n_ranges),
                                                   std::vector<int>(exclude, exclude + (n_exclude > 0 ? n_exclude : 0)), lambda, pool,
                                                   max_per_artist),
                    out, scores, cap);
}
// Recommender::setPriors (one per song) and Recommender::recommendQuery, the Query's fields as flat arrays (a count of 0: empty).
int shim_set_priors(void* h, const float* priors) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return c->rec.setPriors(std::vector<float>(priors, priors + c->rec.getSongCount())) ? 1 : 0;
}
int64_t shim_query(void* h, const int* songs, int n_songs, const float* weights, int n_weights, const int* features, const float* lo,
                   const float* hi, int n_ranges, const int* exclude, int n_exclude, const int* genres, int n_genres, int diverse,
                   float lambda, int pool, int max_per_artist, float prior_weight, const float* scales, int n_scales, int euclidean,
                   int topn, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    Recommender::Query q;
    q.songs.assign(songs, songs + n_songs);
    q.weights.assign(weights, weights + n_weights);
    q.where = ranges(features, lo, hi, n_ranges);
    q.alsoExclude.assign(exclude, exclude + n_exclude);
    q.genreIds.assign(genres, genres + n_genres);
    q.diverse = diverse != 0;
    q.lambda = lambda;
    q.pool = pool;
    q.maxPerArtist = max_per_artist;
    q.priorWeight = prior_weight;
    q.scales.assign(scales, scales + n_scales);
    q.euclidean = euclidean != 0;
    q.topN = topn;
    return giveBack(c, c->rec.recommendQuery(q), out, scores, cap);
}
// The most general recommendForPlaylist overload (genre ids and a prior weight last) and recommendScaled (n_scales 0: none;
// recommendNearest is its euclidean form without scales).
int64_t shim_recommend_for_playlist_general(void* h, const int* songs, int n_songs, const float* weights, int n_weights, int topn,
                                            const int* features, const float* lo, const float* hi, int n_ranges, const int* exclude,
                                            int n_exclude, float lambda, int pool, int max_per_artist, const int* genres, int n_genres,
                                            float prior_weight, int* out, float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    return giveBack(c, c->rec.recommendForPlaylist(std::vector<int>(songs, songs + n_songs), topn, std::vector<float>(weights, weights + n_weights),
                                                   ranges(features, lo, hi, n_ranges), std::vector<int>(exclude, exclude + n_exclude), lambda,
                                                   pool, max_per_artist, std::vector<int>(genres, genres + n_genres), prior_weight),
                    out, scores, cap);
}
int64_t shim_recommend_scaled(void* h, const int* songs, int n_songs, int topn, const float* scales, int n_scales, int euclidean,
                              const int* features, const float* lo, const float* hi, int n_ranges, const int* genres, int n_genres, int* out,
                              float* scores, int64_t cap) {
    Catalogue* c = static_cast<Catalogue*>(h);
    const std::vector<int> s(songs, songs + n_songs), g(genres, genres + n_genres);
    const std::vector<Recommender::FeatureRange> where = ranges(features, lo, hi, n_ranges);
    return giveBack(c, euclidean && n_scales == 0 ? c->rec.recommendNearest(s, topn, where, g)
                                                  : c->rec.recommendScaled(s, topn, std::vector<float>(scales, scales + n_scales), euclidean != 0, where, g),
                    out, scores, cap);
}
int shim_artist_groups(void* h, int* out_n) {
    Catalogue* c = static_cast<Catalogue*>(h);
    std::vector<std::string> artists;
    for (const Song& s : c->songs) artists.push_back(s.artists);
    const std::vector<int> g = Recommender::artistGroupIds(artists);
    for (size_t i = 0; i < g.size(); ++i) out_n[i] = g[i];
    return 1;
}
int shim_similarities(void* h, int idx, float* out_n) {
    Catalogue* c = static_cast<Catalogue*>(h);
    std::vector<float> v;
    if (!c->rec.similarities(idx, v)) return 0;
    std::memcpy(out_n, v.data(), v.size() * sizeof(float));
    return 1;
}

}  // extern "C"
