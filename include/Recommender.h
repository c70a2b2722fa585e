// Recommender.h — the reference's public class API over the MI355X engine.
//
// Drop-in for the reference's Recommender.h:28-83: same class name, same
// public member signatures and the public `Recommendation` struct
// (Recommender.h:12-22), so the reference's main.cpp compiles against this
// header unchanged.  The private part is an opaque pointer: all device state
// lives behind the C-ABI in include/mi355rec.h.
//
// Behavioural contract:
//  - initialize(): false for an empty song list (Recommender.cu:103-106).  On a
//    host WITHOUT a HIP device it does what the reference does (Recommender.cu:
//    117-127,176-181): prints the reference's fallback lines, serves the
//    catalogue from the product's own CPU backend (csrc/cpu_backend.cpp, behind
//    mi355rec_create_placed) and returns true with isGPUEnabled() == false.  On a
//    host WITH a device nothing ever falls back: a failed HIP call is an error.
//  - recommendByIndex(): ids of the topN most cosine-similar songs, best
//    first, the query excluded by index; min(topN, N-1) results; {} plus the
//    reference's stderr text for an uninitialised object or a bad index.
//    topN <= 0 returns {} (the reference crashes).
//    Order inside runs of exactly equal scores is ascending index (the
//    reference's is a heap artefact).
//  - recommend()/recommendByName(): the reference's lookup rules
//    (Recommender.cu:320-354): exact id; name = case-insensitive exact match
//    first, else first case-insensitive substring match.
#ifndef RECOMMENDER_H
#define RECOMMENDER_H

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "Song.h"

struct Recommendation {
    int songIndex;
    float similarity;

    Recommendation() : songIndex(-1), similarity(0.0f) {}
    Recommendation(int idx, float sim) : songIndex(idx), similarity(sim) {}

    // inverted on purpose, as in the reference: a std::priority_queue of
    // Recommendation keeps the LOWEST similarity on top
    bool operator<(const Recommendation& other) const { return similarity > other.similarity; }
};

class Recommender {
public:
    Recommender();
    ~Recommender();
    Recommender(const Recommender&) = delete;
    Recommender& operator=(const Recommender&) = delete;

    bool initialize(const std::vector<Song>& songs);

    std::vector<int> recommend(const std::string& trackId, int topN);
    std::vector<int> recommendByName(const std::string& trackName, int topN);
    std::vector<int> recommendByIndex(int songIndex, int topN);

    bool isInitialized() const;
    bool isGPUEnabled() const;
    int getSongCount() const;

    // Extension: the same initialisation from what DataManager::loadCatalogue read —
    // the row-major N x 12 matrix goes to the GPUs as it is, ids / names feed the
    // lookups; no vector<Song> is ever built (the reference deep-copies it,
    // Recommender.cu:109, then flattens it, :162-167).
    bool initialize(const std::vector<float>& features, const std::vector<std::string>& trackIds,
                    const std::vector<std::string>& trackNames);

    // Extensions (not in the reference): the scores of the last
    // recommendByIndex result, and the full score vector of one query row
    // (what the reference's private calculateSimilarities produced).
    const std::vector<float>& lastScores() const;
    bool similarities(int songIndex, std::vector<float>& out);

    // Extension: genre-restricted recommendations.  recommendByIndexInGenres returns the ids of the topN songs most
    // similar to songIndex among the songs whose genre id is in genreIds (same checks, messages, order and exclusion
    // as recommendByIndex; lastScores() is filled the same way).  initialize(songs) keeps the songs' genre ids;
    // after the matrix overload of initialize, setGenreIds gives them (one per song; -1 = no genre).  The labels
    // reach the engine on the first genre-restricted call.
    bool setGenreIds(const std::vector<int>& genreIds);
    std::vector<int> recommendByIndexInGenres(int songIndex, int topN, const std::vector<int>& genreIds);

    // Extension: playlist recommendations.  recommendForPlaylist returns the ids of the topN songs whose mean similarity
    // to the songs of songIndices (1 to 32 of them, duplicates counting twice) is the highest, the playlist's songs and
    // alsoExclude (up to 1024 ids) left out; same messages and {} on bad input as recommendByIndex, lastScores() filled.
    // topN is capped at the songs that can be returned; above 1024 it is refused.
    std::vector<int> recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<int>& alsoExclude = {});

    // Extension: feature-range filters.  Only songs whose feature `feature` (0..11 in Song.h order: danceability, energy,
    // key, loudness, mode, speechiness, acousticness, instrumentalness, liveness, valence, tempo, genre id) lies in
    // [lo, hi] are returned, in the units of the matrix (songs_data.bin: normalised to [0, 1]).  Several ranges on one
    // feature intersect; an empty range list filters nothing.  recommendByIndexWhere is recommendByIndex among the songs that
    // pass every range (same checks, messages and lastScores(); topN above 1024 is refused); the overload of
    // recommendForPlaylist does the same for a playlist.  A feature outside 0..11, a NaN bound, lo > hi or ranges on one
    // feature that do not overlap give {} and a message.
    struct FeatureRange {
        int feature;
        float lo, hi;
    };
    std::vector<int> recommendByIndexWhere(int songIndex, int topN, const std::vector<FeatureRange>& where);
    std::vector<int> recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<FeatureRange>& where,
                                          const std::vector<int>& alsoExclude);

    // Extension: weighted playlists (likes and dislikes).  The overload of recommendForPlaylist takes one weight per song of
    // songIndices, of any sign: a song's similarity counts w times, a negative weight pushes results away from that song,
    // and the score is sum(w_k * similarity_k) / sum(|w_k|), in [-1, 1] (lastScores()).  The playlist's songs are never
    // returned, whatever their weight.  `where` and `alsoExclude` as above (both may be empty).  A weight list whose length
    // differs from the songs', a NaN or infinite weight, |w| > 1e6 or weights that are all zero give {} and a message.
    // recommendForTaste is the common case: the liked songs at weight +1, the disliked ones at -dislikeWeight
    // (dislikeWeight >= 0; liked.size() + disliked.size() <= 32, at least one liked song).
    std::vector<int> recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                                          const std::vector<FeatureRange>& where, const std::vector<int>& alsoExclude);
    std::vector<int> recommendForTaste(const std::vector<int>& liked, const std::vector<int>& disliked, int topN,
                                       float dislikeWeight = 0.5f, const std::vector<FeatureRange>& where = {},
                                       const std::vector<int>& alsoExclude = {});

    // Extension: diversified recommendations (maximal marginal relevance).  The `pool` most similar songs are found as
    // above; topN of them are then picked one by one, each pick maximising
    //     lambda * similarity - (1 - lambda) * (its largest similarity to a song already picked),
    // so lambda = 1 is the plain result and smaller values spread the results out (0.7 is a usual choice).  The ids come
    // in pick order; lastScores() holds their similarity (the relevance, not the mmr value).  pool = 0 means
    // min(1024, max(topN, 4 * topN)); otherwise topN <= pool <= 1024.  recommendDiverse is recommendByIndex diversified
    // (same checks and messages; `where` as in recommendByIndexWhere); the overload of recommendForPlaylist takes weights
    // (empty: none), `where` and alsoExclude (both may be empty) as above.  lambda NaN or outside [0, 1], a pool below topN
    // or above 1024 give {} and a message.
    std::vector<int> recommendDiverse(int songIndex, int topN, float lambda, int pool = 0, const std::vector<FeatureRange>& where = {});
    std::vector<int> recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                                          const std::vector<FeatureRange>& where, const std::vector<int>& alsoExclude, float lambda,
                                          int pool = 0);

    // Extension: at most maxPerArtist results per artist (group caps).  initialize(songs) derives one group id per song from
    // Song::artists: the key is the bytes before the first ';' (the primary artist of the CSV's artists column), matched
    // exactly; an empty key means no group (the song is never capped).  After the matrix overload of initialize,
    // setGroupIds gives the ids (one per song; >= 0 a group, -1 none); artistGroupIds derives them from artists strings
    // the same way.  The groups reach the engine on the first capped call.  recommendByIndexCapped is recommendDiverse
    // with the cap (lambda = 1: the most similar songs in order, those beyond an artist's cap skipped); pool = 0 means
    // min(1024, max(topN, 8 * topN)).  Fewer than topN results come back when the pool holds no more eligible songs: raise
    // pool.  The overload of recommendForPlaylist takes the cap after pool.  maxPerArtist < 1 or unknown groups give {} and
    // a message; everything else as for the diversified forms.
    // Extension: the whole family within genres.  This most general overload of recommendForPlaylist takes, last, the genre
    // ids the results must come from (as recommendByIndexInGenres: the songs' genres are those of initialize(songs) or
    // setGenreIds; the playlist's own songs may belong to any genre).  Empty: no restriction, the call as before (maxPerArtist
    // < 1 stays an error there).  With genre ids this overload is the whole family, so maxPerArtist = 0 is accepted and asks
    // for no cap: the diversified call, and with lambda = 1 the plain top-N within the genres (no pool, no re-rank).  A single song within
    // genres with a filter, diversity or a cap is the one-song playlist {songIndex}.
    // Extension: row priors.  setPriors gives every song one float in [-1, 1] (popularity, freshness, an editorial boost; one
    // per song, every value finite); the last argument of the general overload, priorWeight, then ranks by
    // similarity + priorWeight * prior (|priorWeight| <= 4; negative demotes; lastScores() holds the blended values).
    // priorWeight = 0 (the default) is the call as before.  Like genre ids, a prior weight makes the general overload the whole
    // family: maxPerArtist = 0 then asks for no cap.  The priors reach the engine on the first call that uses them.
    bool setPriors(const std::vector<float>& priors);
    static std::vector<int> artistGroupIds(const std::vector<std::string>& artists);
    bool setGroupIds(const std::vector<int>& groupIds);
    std::vector<int> recommendByIndexCapped(int songIndex, int topN, int maxPerArtist, float lambda = 1.0f, int pool = 0,
                                            const std::vector<FeatureRange>& where = {});
    std::vector<int> recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                                          const std::vector<FeatureRange>& where, const std::vector<int>& alsoExclude, float lambda,
                                          int pool, int maxPerArtist, const std::vector<int>& genreIds = {}, float priorWeight = 0.0f);

    // Extension: nearest songs by Euclidean distance (the reference's "Additional Metrics: Euclidean").  recommendNearest
    // returns the ids of the topN songs NEAREST to the songs of songIndices (1 to 32; never returned themselves) over the 12
    // features of the matrix, nearest first; lastScores() holds the DISTANCES (ascending): for one song the Euclidean distance,
    // for several the root-mean-square distance to them, which ranks as the distance to their centroid does.  Cosine ignores
    // magnitude; on the min-max normalised matrix of songs_data.bin the distance does not.  `where` and `genreIds` as above
    // (both may be empty).  Weights, diversity, caps and priors are not served with this metric.  Same messages and {} on bad
    // input as recommendForPlaylist.
    std::vector<int> recommendNearest(const std::vector<int>& songIndices, int topN, const std::vector<FeatureRange>& where = {},
                                      const std::vector<int>& genreIds = {});

    // Extension: feature scales (include/mi355rec_diag.h, "FEATURE SCALES").  recommendScaled is the playlist recommendation
    // (euclidean = false: lastScores() holds the scaled cosine means, best first) or recommendNearest (euclidean = true:
    // lastScores() holds the distances) with every feature j of the songs multiplied by scales[j] first: 12 non-negative
    // factors in Song.h order, 0 ignores a feature, 2 makes it count double; an empty vector is the unscaled call.  `where`
    // still tests the stored features.  Same messages and {} on bad input as recommendNearest; the engine refuses scales that
    // are negative, not finite, above 1024 or all zero.
    std::vector<int> recommendScaled(const std::vector<int>& songIndices, int topN, const std::vector<float>& scales, bool euclidean,
                                     const std::vector<FeatureRange>& where = {}, const std::vector<int>& genreIds = {});

    // Extension: row sets (include/mi355rec_diag.h, "ROW SETS").  setRowSet gives the songs a listener has already heard
    // (only = false: they are never returned) or the candidates to rank within (only = true: only they are returned); any
    // number of them, duplicates allowed, where alsoExclude holds at most 1024.  The set applies to every recommendForPlaylist,
    // recommendNearest and recommendScaled call, and to the single-song forms that are one-song playlists (recommendByIndexWhere,
    // recommendDiverse, recommendByIndexCapped), until clearRowSet() or the next setRowSet, beside everything those calls take; it
    // costs one bit per song on the host and on every device.  recommend(), recommendByIndex() and recommendByName() (the
    // reference's own single-query path) are unchanged.  An index outside the songs gives false and a message, and the set as
    // it was.
    bool setRowSet(const std::vector<int>& songIndices, bool only = false);
    void clearRowSet();

    // Extension: candidate lists (include/mi355rec_diag.h, "CANDIDATE LISTS").  setCandidates gives the songs to rank within, the
    // output of a first stage: any order, duplicates allowed, at most 1 048 576.  Where setRowSet(..., true) keeps one bit per song
    // and every request reads the whole catalogue, a request with a list reads only the listed songs; the results are the same.  The
    // list applies to the calls the row set applies to, until clearCandidates() or the next setCandidates, and goes with a row set
    // (setRowSet(history) and setCandidates(candidates): the candidates not heard yet).  An empty list is a list: nothing is
    // returned.  An index outside the songs gives false and a message, and the list as it was.
    bool setCandidates(const std::vector<int64_t>& songIndices);
    void clearCandidates();

    // Extension: one description of a request.  Every method above that takes a playlist (and recommendByIndexWhere,
    // recommendDiverse, recommendByIndexCapped, which take the one-song playlist) fills a Query and runs it through
    // recommendQuery; a caller may do so itself and combine what no overload combines (scales with alsoExclude, say).  The
    // fields mean what the parameters of those methods mean; messages and {} on bad input are theirs.  maxPerArtist = 0 asks
    // for no cap; a cap without `diverse` is the plain order with the cap (lambda stays 1); `diverse` with lambda = 1 within genres
    // or with a prior weight is the plain request (the same result without a pool).  With euclidean set, lastScores()
    // holds distances, and weights, diverse, maxPerArtist and priorWeight are refused.  The row set of setRowSet applies.
    // anyOf (include/mi355rec_diag.h, "ANY-OF REQUESTS"): songs rank by their BEST similarity among `songs` ("like any of these")
    // instead of the mean; lastScores() holds that similarity and lastMatchedSongs() the song of `songs` each result matched.  With
    // anyOf, weights, diverse, maxPerArtist, priorWeight, scales and euclidean are refused with a message and {}, and so are a set
    // candidate list (setCandidates) and scoreSongs.  The row set of setRowSet applies.
    // manhattan (include/mi355rec_diag.h, "MANHATTAN REQUESTS"): songs rank by their mean L1 distance to `songs`, nearest first;
    // lastScores() holds the distances.  With manhattan, weights, diverse, maxPerArtist, priorWeight, scales, euclidean and anyOf are
    // refused with a message and {}, and so are a set candidate list (setCandidates) and scoreSongs.  The row set of setRowSet applies.
    // atLeast / within (include/mi355rec_diag.h, "BOUNDED REQUESTS"): only songs that are good enough, and how many there are.
    // query.atLeast(s) keeps the songs whose similarity (the plain mean) is >= s; query.within(r) sets euclidean and keeps the songs
    // whose distance is <= r.  The results are the leading matches, at most topN of them (topN = 0 is allowed: count only), and
    // lastMatchCount() holds the exact number of matching songs.  With a bound, weights, diverse, maxPerArtist, priorWeight, scales,
    // anyOf and manhattan are refused with a message and {}, and so are a set candidate list and scoreSongs.  The row set applies.
    // jaccard (include/mi355rec_diag.h, "JACCARD REQUESTS"): songs rank by their mean weighted (Ruzicka) Jaccard similarity to `songs`,
    // sum_j min(q_j, x_j) / sum_j max(q_j, x_j), most similar first; lastScores() holds the similarities.  With jaccard, weights,
    // diverse, maxPerArtist, priorWeight, scales, euclidean, manhattan, anyOf and a bound are refused with a message and {}, and so
    // are a set candidate list (setCandidates) and scoreSongs.  The row set of setRowSet applies.
    struct Query {
        std::vector<int> songs;            // 1 to 32
        std::vector<float> weights;        // one per song, or none
        std::vector<FeatureRange> where;
        std::vector<int> alsoExclude;      // up to 1024
        std::vector<int> genreIds;         // empty: every genre
        bool diverse = false;              // re-rank the `pool` best by maximal marginal relevance with `lambda`
        float lambda = 1.0f;
        int pool = 0;                      // 0: min(1024, 4 * topN), with a cap 8 * topN
        int maxPerArtist = 0;
        float priorWeight = 0.0f;
        std::vector<float> scales;         // 12, or none
        bool euclidean = false;
        int topN = 10;
        bool anyOf = false;
        bool manhattan = false;
        bool bounded = false;              // set by atLeast / within: `bound` is a score floor, or (euclidean) a radius
        float bound = 0.0f;
        Query& atLeast(float score) { bounded = true, euclidean = false, bound = score; return *this; }
        Query& within(float radius) { bounded = true, euclidean = true, bound = radius; return *this; }
        bool jaccard = false;
    };
    std::vector<int> recommendQuery(const Query& query);
    // Per result of the last recommendQuery with anyOf: the catalogue index of the matched song of query.songs (the first of them
    // that attains the result's score).  Empty after any other call.
    const std::vector<int>& lastMatchedSongs() const;
    // The number of songs that matched the bound of the last recommendQuery with atLeast / within (whatever its topN); -1 after any
    // other call and after one that failed.
    long long lastMatchCount() const;

    // Extension: candidate scores (include/mi355rec_diag.h, "CANDIDATE SCORES").  scoreSongs gives what `query` is worth at every
    // song of songIndices, in their order (duplicates allowed, at most 1 048 576): the score (with euclidean the distance)
    // recommendQuery would report for that song, bit for bit; for a blender that mixes a first stage's score with this one, or "how
    // similar is song A to song B".  A song the query can never return (one of query.songs or alsoExclude, outside where or genreIds,
    // rejected by the row set) gets NaN, and 0 in *admissible (1 otherwise) where that is given.  topN is ignored; diverse and
    // maxPerArtist are refused with a message and {} (a re-ranked order has no value per song), as is an index outside the songs.
    // The row set of setRowSet applies; the list of setCandidates does not.  lastScores() is left as it was.
    std::vector<float> scoreSongs(const Query& query, const std::vector<int64_t>& songIndices, std::vector<char>* admissible = nullptr);

    // Extension: in-place updates (include/mi355rec_diag.h, "ROW UPDATES").  updateSongs gives the songs at `indices` (distinct,
    // inside the catalogue) new features: 12 floats per song in Song.h order, features[12 * i ..] for indices[i].  Every later
    // recommendation answers as if the catalogue had been initialised with the new features; ids, names, genre ids, groups,
    // priors and the row set stay as they are.  A wrong length, an index outside the songs or one named twice give false and a
    // message, and the catalogue as it was.  An empty list succeeds.
    bool updateSongs(const std::vector<int>& indices, const std::vector<float>& features);

    struct Impl;   // opaque: defined in Recommender.cpp

private:
    Impl* impl_;
};

#endif  // RECOMMENDER_H
