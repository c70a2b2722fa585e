// Recommender.cpp — host shim: the reference's Recommender class on top of the
// C-ABI (include/mi355rec.h).  Replaces Recommender.cu:80-372; every method
// names the reference lines whose observable behaviour it keeps.
#include "Recommender.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <iostream>
#include <unordered_map>

#include "mi355rec_diag.h"   // (the core + mi355rec_sharded_note / _placement for the messages)

namespace {
// A per-song array that the engine is handed by the first call that needs it (initialize costs what it costs without it): the
// values (one per song; empty: not known) and whether THIS engine has them yet.
template <class T>
struct PerSong {
    std::vector<T> values;
    bool uploaded = false;
    void set(const std::vector<T>& v) { values = v, uploaded = false; }
};
}  // namespace

struct Recommender::Impl {
    bool initialized = false;
    bool gpuEnabled = false;
    int numSongs = 0;
    mi355rec_sharded_t* engine = nullptr;   // the catalogue on the node's GPUs (placement: include/mi355rec.h) — or, without any, on the CPU backend
    int numDevices = 0;

    // Only what the lookups need is kept (the reference deep-copies every Song,
    // Recommender.cu:109).  `byId` maps a track id to its FIRST row, which is
    // what the reference's linear scan returns; `lowerNames` is lowered once
    // instead of once per row per query (Recommender.cu:340-351).
    std::vector<std::string> lowerNames;
    std::unordered_map<std::string, int> byId;

    PerSong<int> genres;     // genre ids (-1 = none): the first genre-restricted query uploads them
    PerSong<int> groups;     // group ids (-1 = none): the first capped query
    PerSong<float> priors;   // setPriors: the first query with a prior weight

    // setRowSet: the engine's set (null: none) and its mode.  It belongs to `engine`: dropRowSet before the engine goes.
    mi355rec_rowset_t* rowSet = nullptr;
    bool rowSetOnly = false;
    // setCandidates: the candidate list of the requests (hasCandidates: an empty list is a list).
    std::vector<int64_t> candidates;
    bool hasCandidates = false;
    void dropRowSet() {
        mi355rec_rowset_destroy(rowSet);
        rowSet = nullptr;
        rowSetOnly = false;
    }

    std::vector<int64_t> idxBuf;
    std::vector<float> scoreBuf;
    std::vector<float> lastScores;
    std::vector<int> lastMatched;   // Query::anyOf: the matched song of every result of the last such query
    long long lastMatchCount = -1;  // Query::atLeast / within: the matching songs of the last such query
};

namespace {

std::string toLower(const std::string& str) {  // Recommender.cu:329-334
    std::string result = str;
    for (char& c : result) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
    return result;
}

}  // namespace

Recommender::Recommender() : impl_(new Impl()) {}

Recommender::~Recommender() {  // Recommender.cu:86-98
    impl_->dropRowSet();
    if (impl_->engine) mi355rec_sharded_destroy(impl_->engine);
    delete impl_;
}

namespace {

// Shared tail of the two initialize() overloads: lookup tables + upload.
bool startEngine(Recommender::Impl* impl, const float* matrix, size_t n);

}  // namespace

bool Recommender::initialize(const std::vector<Song>& songs) {  // Recommender.cu:100-182
    std::cout << "Initializing GPU-accelerated recommender..." << std::endl;
    if (songs.empty()) {  // :103-106
        std::cerr << "Error: Empty song database" << std::endl;
        return false;
    }
    // AoS -> row-major N x 12 (the reference's staging matrix, :162-167)
    std::vector<float> matrix(songs.size() * FEATURE_COUNT);
    impl_->lowerNames.clear();
    impl_->lowerNames.reserve(songs.size());
    impl_->byId.clear();
    impl_->byId.reserve(songs.size() * 2);
    impl_->genres.values.resize(songs.size());
    {
        std::vector<std::string> artists;
        artists.reserve(songs.size());
        for (const Song& s : songs) artists.push_back(s.artists);
        impl_->groups.values = artistGroupIds(artists);
    }
    for (size_t i = 0; i < songs.size(); ++i) {
        std::copy(songs[i].features, songs[i].features + FEATURE_COUNT, matrix.begin() + i * FEATURE_COUNT);
        impl_->genres.values[i] = songs[i].genre_id;
        impl_->lowerNames.push_back(toLower(songs[i].track_name));
        impl_->byId.emplace(songs[i].track_id, static_cast<int>(i));  // keeps the first
    }
    return startEngine(impl_, matrix.data(), songs.size());
}

bool Recommender::initialize(const std::vector<float>& features, const std::vector<std::string>& trackIds,
                             const std::vector<std::string>& trackNames) {
    std::cout << "Initializing GPU-accelerated recommender..." << std::endl;
    if (trackIds.empty()) {
        std::cerr << "Error: Empty song database" << std::endl;
        return false;
    }
    if (features.size() != trackIds.size() * FEATURE_COUNT || trackNames.size() != trackIds.size()) {
        std::cerr << "Error: feature matrix / id / name sizes disagree" << std::endl;
        return false;
    }
    impl_->lowerNames.clear();
    impl_->lowerNames.reserve(trackIds.size());
    impl_->byId.clear();
    impl_->byId.reserve(trackIds.size() * 2);
    for (size_t i = 0; i < trackIds.size(); ++i) {
        impl_->lowerNames.push_back(toLower(trackNames[i]));
        impl_->byId.emplace(trackIds[i], static_cast<int>(i));
    }
    impl_->genres.values.clear();
    impl_->groups.values.clear();
    return startEngine(impl_, features.data(), trackIds.size());
}

namespace {

bool startEngine(Recommender::Impl* impl, const float* matrix, size_t n) {
    impl->dropRowSet();   // (a set is the engine's that made it: after a re-initialisation the class holds none)
    impl->candidates.clear();   // (... and no candidate list: its ids were songs of the catalogue before)
    impl->hasCandidates = false;
    if (impl->engine) {
        mi355rec_sharded_destroy(impl->engine);
        impl->engine = nullptr;
    }
    impl->initialized = false;
    impl->gpuEnabled = false;
    impl->genres.uploaded = impl->groups.uploaded = impl->priors.uploaded = false;   // (the new engine has none of them)
    impl->numSongs = static_cast<int>(n);
    // The reference pins device 0 (Recommender.cu:124).  Here the library places the catalogue itself: one device up
    // to 7.9 M rows, row-sharded over as many as keep 4 M rows per shard beyond that (one process, one stream per
    // device, xGMI peer stores or one RCCL all-gather of the per-shard top-N keys: include/mi355rec.h, "PLACEMENT").
    // Without any HIP device the handle is served by the product's own CPU backend, as the reference falls back to
    // its CPU loop (:117-127,176-181).
    const int rc = mi355rec_create_placed(matrix, static_cast<int64_t>(n), FEATURE_COUNT, nullptr, /*n_devices=*/0,
                                          MI355REC_PLACEMENT_AUTO, &impl->engine);
    if (rc != MI355REC_OK) {   // a device is there but could not be used (or memory ran out): say why and give up
        std::cerr << "[GPU Disabled] " << mi355rec_sharded_last_error(nullptr) << std::endl;
        std::cerr << "Error: the recommender could not be initialized" << std::endl;
        return false;
    }
    impl->initialized = true;
    if (mi355rec_sharded_placement(impl->engine) == MI355REC_PLACEMENT_CPU) {
        // the reference's own lines for this case (Recommender.cu:120-121,177)
        std::cerr << "[GPU Disabled] HIP runtime not available: no HIP device visible" << std::endl;
        std::cerr << "Falling back to CPU similarity computation." << std::endl;
        std::cout << "Operating in CPU fallback mode (cosine similarity on CPU)." << std::endl;
        impl->gpuEnabled = false;
        impl->numDevices = 0;
        return true;
    }
    mi355rec_sharded_info(impl->engine, &impl->numDevices, nullptr, nullptr, nullptr, nullptr);
    impl->gpuEnabled = true;
    // the reference's stdout line, byte for byte (Recommender.cu:172); the placement note goes to stderr
    std::cout << "Successfully initialized with " << impl->numSongs << " songs on GPU" << std::endl;
    if (impl->numDevices > 1) {
        std::cerr << "[mi355rec] catalogue row-sharded over " << impl->numDevices << " devices" << std::endl;
        const char* note = mi355rec_sharded_note(impl->engine);
        if (note && note[0]) std::cerr << "[mi355rec] " << note << std::endl;
    }
    return true;
}

}  // namespace

namespace {

// recommendByIndex's checks (Recommender.cu:275-292); false: nothing to ask the engine (the message, if any, is out).
bool checkQuery(const Recommender::Impl* impl, int songIndex, int& topN) {
    if (!impl->initialized) {
        std::cerr << "Error: Recommender not initialized" << std::endl;
        return false;
    }
    if (songIndex < 0 || songIndex >= impl->numSongs) {
        std::cerr << "Error: Invalid song index: " << songIndex << std::endl;
        return false;
    }
    if (topN <= 0) {
        std::cerr << "Error: topN must be positive" << std::endl;
        return false;
    }
    // The reference's heap never holds more than N-1 entries (Recommender.cu:296-305):
    // a larger topN returns N-1 results, and must not size any buffer.
    if (topN > impl->numSongs - 1) topN = impl->numSongs - 1;
    return topN > 0;   // (a one-song catalogue has nothing to recommend)
}

}  // namespace

std::vector<int> Recommender::recommendByIndex(int songIndex, int topN) {  // Recommender.cu:275-318
    if (!checkQuery(impl_, songIndex, topN)) return {};
    impl_->idxBuf.assign(static_cast<size_t>(topN), -1);
    impl_->scoreBuf.assign(static_cast<size_t>(topN), 0.0f);
    int count = 0;
    const int rc = mi355rec_sharded_query_row_topn(impl_->engine, songIndex, topN, impl_->idxBuf.data(),
                                                   impl_->scoreBuf.data(), &count);
    if (rc != MI355REC_OK) {
        std::cerr << "Error: " << mi355rec_sharded_last_error(impl_->engine) << std::endl;
        return {};
    }
    std::vector<int> results(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) results[i] = static_cast<int>(impl_->idxBuf[i]);
    impl_->lastScores.assign(impl_->scoreBuf.begin(), impl_->scoreBuf.begin() + count);
    return results;
}

std::vector<int> Recommender::artistGroupIds(const std::vector<std::string>& artists) {
    std::vector<int> ids(artists.size(), -1);
    std::unordered_map<std::string, int> seen;   // primary artist -> id, in order of first appearance
    for (size_t i = 0; i < artists.size(); ++i) {
        const std::string key = artists[i].substr(0, artists[i].find(';'));
        if (key.empty()) continue;
        ids[i] = seen.emplace(key, static_cast<int>(seen.size())).first->second;
    }
    return ids;
}

bool Recommender::setGroupIds(const std::vector<int>& groupIds) {
    if (!impl_->initialized || groupIds.size() != static_cast<size_t>(impl_->numSongs)) {
        std::cerr << "Error: one group id per song is needed" << std::endl;
        return false;
    }
    for (int g : groupIds)
        if (g < -1) {
            std::cerr << "Error: group id " << g << ": a group id is >= 0, or -1 for no group" << std::endl;
            return false;
        }
    impl_->groups.set(groupIds);
    return true;
}

bool Recommender::setPriors(const std::vector<float>& priors) {
    if (!impl_->initialized || priors.size() != static_cast<size_t>(impl_->numSongs)) {
        std::cerr << "Error: one prior per song is needed" << std::endl;
        return false;
    }
    for (size_t i = 0; i < priors.size(); ++i)
        if (!(std::fabs(priors[i]) <= 1.0f)) {   // (NaN too)
            std::cerr << "Error: prior " << priors[i] << " of song " << i << ": a prior is finite with |p| <= 1" << std::endl;
            return false;
        }
    impl_->priors.set(priors);
    return true;
}

bool Recommender::updateSongs(const std::vector<int>& indices, const std::vector<float>& features) {
    if (!impl_->initialized) {
        std::cerr << "Error: Recommender not initialized" << std::endl;
        return false;
    }
    if (features.size() != indices.size() * static_cast<size_t>(MI355REC_DIM)) {
        std::cerr << "Error: " << MI355REC_DIM << " features per updated song are needed" << std::endl;
        return false;
    }
    const std::vector<int64_t> rows(indices.begin(), indices.end());
    if (mi355rec_sharded_update_rows(impl_->engine, rows.data(), static_cast<int64_t>(rows.size()), features.data()) != MI355REC_OK) {
        std::cerr << "Error: " << mi355rec_sharded_last_error(impl_->engine) << std::endl;
        return false;
    }
    return true;
}

bool Recommender::setRowSet(const std::vector<int>& songIndices, bool only) {
    if (!impl_->initialized) {
        std::cerr << "Error: Recommender not initialized" << std::endl;
        return false;
    }
    const std::vector<int64_t> ids(songIndices.begin(), songIndices.end());
    mi355rec_rowset_t* fresh = nullptr;
    if (mi355rec_sharded_rowset_create(impl_->engine, ids.data(), static_cast<int64_t>(ids.size()), &fresh) != MI355REC_OK) {
        std::cerr << "Error: " << mi355rec_sharded_last_error(impl_->engine) << std::endl;
        return false;
    }
    impl_->dropRowSet();
    impl_->rowSet = fresh;
    impl_->rowSetOnly = only;
    return true;
}

void Recommender::clearRowSet() { impl_->dropRowSet(); }

bool Recommender::setCandidates(const std::vector<int64_t>& songIndices) {
    if (!impl_->initialized) {
        std::cerr << "Error: Recommender not initialized" << std::endl;
        return false;
    }
    if (songIndices.size() > static_cast<size_t>(MI355REC_MAX_CANDIDATES)) {
        std::cerr << "Error: " << songIndices.size() << " candidates: at most " << MI355REC_MAX_CANDIDATES << " are taken" << std::endl;
        return false;
    }
    for (int64_t id : songIndices)
        if (id < 0 || id >= impl_->numSongs) {
            std::cerr << "Error: candidate list: id " << id << " out of [0, " << impl_->numSongs << ")" << std::endl;
            return false;
        }
    impl_->candidates = songIndices;
    impl_->hasCandidates = true;
    return true;
}

void Recommender::clearCandidates() {
    impl_->candidates.clear();
    impl_->hasCandidates = false;
}

namespace {
// The per-request extras of a call (FEATURE SCALES, ROW SETS): the scales (null: none) and the row set of setRowSet (none: a null
// pointer; an ext of two null pointers is the plain request).
mi355rec_request_ext_t requestExt(const Recommender::Impl* impl, const float* scales) {
    mi355rec_request_ext_t ext{};
    ext.size = sizeof ext;
    ext.rowset_mode = impl->rowSetOnly ? MI355REC_ROWSET_ONLY : MI355REC_ROWSET_EXCLUDE;
    ext.feature_scales = scales;
    ext.rowset = impl->rowSet;
    return ext;
}
}  // namespace

bool Recommender::setGenreIds(const std::vector<int>& genreIds) {
    if (!impl_->initialized || genreIds.size() != static_cast<size_t>(impl_->numSongs)) {
        std::cerr << "Error: one genre id per song is needed" << std::endl;
        return false;
    }
    for (int g : genreIds)
        if (g < -1 || g >= MI355REC_MAX_LABELS) {
            std::cerr << "Error: genre id " << g << " out of [-1, " << MI355REC_MAX_LABELS << ")" << std::endl;
            return false;
        }
    impl_->genres.set(genreIds);
    return true;
}

namespace {
// The first query that needs a per-song array hands it to the engine through `set`; what / setter: for the message when the
// array is not known.
template <class T>
bool ensureUploaded(Recommender::Impl* impl, PerSong<T>& a, int (*set)(mi355rec_sharded_t*, const T*, int64_t), const char* what,
                    const char* setter) {
    if (a.uploaded) return true;
    if (a.values.size() != static_cast<size_t>(impl->numSongs)) {
        std::cerr << "Error: the songs' " << what << " are not known (" << setter << ")" << std::endl;
        return false;
    }
    if (set(impl->engine, a.values.data(), impl->numSongs) != MI355REC_OK) {
        std::cerr << "Error: " << mi355rec_sharded_last_error(impl->engine) << std::endl;
        return false;
    }
    a.uploaded = true;
    return true;
}
bool ensureGenres(Recommender::Impl* impl) { return ensureUploaded(impl, impl->genres, mi355rec_sharded_set_labels, "genre ids", "setGenreIds"); }
bool ensureGroups(Recommender::Impl* impl) { return ensureUploaded(impl, impl->groups, mi355rec_sharded_set_groups, "group ids", "setGroupIds"); }
bool ensurePriors(Recommender::Impl* impl) { return ensureUploaded(impl, impl->priors, mi355rec_sharded_set_priors, "priors", "setPriors"); }
}  // namespace

std::vector<int> Recommender::recommendByIndexInGenres(int songIndex, int topN, const std::vector<int>& genreIds) {
    if (!checkQuery(impl_, songIndex, topN)) return {};
    if (genreIds.empty()) {
        std::cerr << "Error: no genre to recommend from" << std::endl;
        return {};
    }
    if (!ensureGenres(impl_)) return {};
    impl_->idxBuf.assign(static_cast<size_t>(topN), -1);
    impl_->scoreBuf.assign(static_cast<size_t>(topN), 0.0f);
    int count = 0;
    const int rc = mi355rec_sharded_query_row_topn_labels(impl_->engine, songIndex, genreIds.data(), static_cast<int>(genreIds.size()),
                                                          topN, impl_->idxBuf.data(), impl_->scoreBuf.data(), &count);
    if (rc != MI355REC_OK) {
        std::cerr << "Error: " << mi355rec_sharded_last_error(impl_->engine) << std::endl;
        return {};
    }
    std::vector<int> results(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) results[i] = static_cast<int>(impl_->idxBuf[i]);
    impl_->lastScores.assign(impl_->scoreBuf.begin(), impl_->scoreBuf.begin() + count);
    return results;
}

namespace {

// The ranges as one mi355rec_filter_t (ranges on one feature intersected); false, with a message, when they cannot be.
bool makeFilter(const std::vector<Recommender::FeatureRange>& where, mi355rec_filter_t& f) {
    f.active = 0;
    for (const Recommender::FeatureRange& r : where) {
        if (r.feature < 0 || r.feature >= MI355REC_DIM) {
            std::cerr << "Error: feature index " << r.feature << " out of [0, " << MI355REC_DIM << ")" << std::endl;
            return false;
        }
        if (!(r.lo <= r.hi)) {   // (NaN too)
            std::cerr << "Error: invalid range [" << r.lo << ", " << r.hi << "] on feature " << r.feature << std::endl;
            return false;
        }
        const uint32_t bit = 1u << r.feature;
        if (!(f.active & bit)) {
            f.active |= bit;
            f.lo[r.feature] = r.lo;
            f.hi[r.feature] = r.hi;
            continue;
        }
        f.lo[r.feature] = std::max(f.lo[r.feature], r.lo);
        f.hi[r.feature] = std::min(f.hi[r.feature], r.hi);
        if (f.lo[r.feature] > f.hi[r.feature]) {
            std::cerr << "Error: the ranges on feature " << r.feature << " do not overlap" << std::endl;
            return false;
        }
    }
    return true;
}

// Recommender::recommendQuery: every call that reaches the playlist request or the distance request, and the one place that does.
// rangesLast: `where` is looked at after the songs, topN and the scales instead of first (recommendScaled's order of messages).
// score (scoreSongs; null: a recommendation): the request's value of every song of score->songs instead of its top-N.
struct ScoreSongs {
    const std::vector<int64_t>& songs;
    std::vector<float> values;
    std::vector<uint8_t> admissible;
    bool ok = false;   // the engine has answered: values and admissible hold one entry per song
};
std::vector<int> runQuery(Recommender::Impl* impl, const Recommender::Query& q, bool rangesLast, ScoreSongs* score = nullptr) {
    impl->lastMatchCount = -1;   // (whatever this call turns out to be: only a bounded query that succeeds leaves a count)
    if (!q.weights.empty() && q.weights.size() != q.songs.size()) {
        std::cerr << "Error: " << q.weights.size() << " weights for " << q.songs.size() << " songs (one weight per song, or none)" << std::endl;
        return {};
    }
    mi355rec_filter_t f;
    if (!rangesLast && !makeFilter(q.where, f)) return {};
    if (!impl->initialized) {
        std::cerr << "Error: Recommender not initialized" << std::endl;
        return {};
    }
    if (q.songs.empty() || q.songs.size() > MI355REC_MAX_PLAYLIST) {
        std::cerr << "Error: a playlist holds 1 to " << MI355REC_MAX_PLAYLIST << " songs" << std::endl;
        return {};
    }
    if (q.alsoExclude.size() > MI355REC_MAX_EXCLUDE) {
        std::cerr << "Error: at most " << MI355REC_MAX_EXCLUDE << " songs can be excluded" << std::endl;
        return {};
    }
    const std::vector<int64_t> rows(q.songs.begin(), q.songs.end()), excl(q.alsoExclude.begin(), q.alsoExclude.end());
    for (const std::vector<int64_t>* v : {&rows, &excl})
        for (int64_t i : *v)
            if (i < 0 || i >= impl->numSongs) {
                std::cerr << "Error: Invalid song index: " << i << std::endl;
                return {};
            }
    int topN = score ? 1 : q.topN;   // (scoreSongs ignores topN)
    if (topN < 0 || (topN == 0 && !q.bounded)) {   // ("BOUNDED REQUESTS": topN = 0 counts only)
        std::cerr << "Error: topN must be positive" << std::endl;
        return {};
    }
    if (!q.scales.empty() && q.scales.size() != MI355REC_DIM) {
        std::cerr << "Error: " << q.scales.size() << " feature scales: one per feature, " << MI355REC_DIM << " in all" << std::endl;
        return {};
    }
    if (topN > impl->numSongs) topN = impl->numSongs;   // (the engine pads past what it can return; no buffer beyond the songs)
    if (rangesLast && !makeFilter(q.where, f)) return {};
    const bool capped = q.maxPerArtist != 0, withPrior = q.priorWeight != 0.0f;   // (a NaN weight: the engine refuses it)
    // Within genres or with a prior weight, lambda 1 without a cap is the plain request: its picks are the pool's first topN in
    // order for any pool, so no pool is taken and no re-rank launched (the diversified overload without either keeps its launch).
    const bool plainOrder = q.lambda == 1.0f && (!q.genreIds.empty() || withPrior);
    const bool rerank = capped || (q.diverse && !plainOrder);   // (a cap alone: lambda 1, the plain order with the cap)
    if (score && (q.diverse || capped)) {
        std::cerr << "Error: scoreSongs takes no diversity and no cap (a re-ranked order has no value per song)" << std::endl;
        return {};
    }
    if (q.euclidean && (!q.weights.empty() || rerank || withPrior)) {
        std::cerr << "Error: the Euclidean metric takes no weights, diversity, cap or prior weight" << std::endl;
        return {};
    }
    impl->lastMatched.clear();
    if (q.jaccard) {   // "JACCARD REQUESTS": what the request has no field for, and what is not served with it (ahead of the others' checks)
        if (!q.weights.empty() || rerank || withPrior || !q.scales.empty() || q.euclidean || q.manhattan || q.anyOf || q.bounded) {
            std::cerr << "Error: a Jaccard query takes no weights, diversity, cap, prior weight, feature scales, Euclidean or Manhattan metric, "
                         "any-of matching or bound"
                      << std::endl;
            return {};
        }
        if (impl->hasCandidates) {
            std::cerr << "Error: a Jaccard query takes no candidate list (clearCandidates first)" << std::endl;
            return {};
        }
        if (score) {
            std::cerr << "Error: scoreSongs takes no Jaccard query" << std::endl;
            return {};
        }
    }
    if (q.bounded) {   // "BOUNDED REQUESTS": what the request has no field for, and what is not served with it
        if (!q.weights.empty() || rerank || withPrior || !q.scales.empty() || q.anyOf || q.manhattan) {
            std::cerr << "Error: a bounded query takes no weights, diversity, cap, prior weight, feature scales, any-of matching or Manhattan distance"
                      << std::endl;
            return {};
        }
        if (impl->hasCandidates) {
            std::cerr << "Error: a bounded query takes no candidate list (clearCandidates first)" << std::endl;
            return {};
        }
        if (score) {
            std::cerr << "Error: scoreSongs takes no bounded query" << std::endl;
            return {};
        }
    }
    if (q.anyOf) {   // "ANY-OF REQUESTS": what the request has no field for, and what is not served with it
        if (!q.weights.empty() || rerank || withPrior || !q.scales.empty() || q.euclidean) {
            std::cerr << "Error: an any-of query takes no weights, diversity, cap, prior weight, feature scales or Euclidean metric" << std::endl;
            return {};
        }
        if (impl->hasCandidates) {
            std::cerr << "Error: an any-of query takes no candidate list (clearCandidates first)" << std::endl;
            return {};
        }
        if (score) {
            std::cerr << "Error: scoreSongs takes no any-of query" << std::endl;
            return {};
        }
    }
    if (q.manhattan) {   // "MANHATTAN REQUESTS": what the request has no field for, and what is not served with it
        if (!q.weights.empty() || rerank || withPrior || !q.scales.empty() || q.euclidean || q.anyOf) {
            std::cerr << "Error: a Manhattan query takes no weights, diversity, cap, prior weight, feature scales, Euclidean metric or any-of matching"
                      << std::endl;
            return {};
        }
        if (impl->hasCandidates) {
            std::cerr << "Error: a Manhattan query takes no candidate list (clearCandidates first)" << std::endl;
            return {};
        }
        if (score) {
            std::cerr << "Error: scoreSongs takes no Manhattan query" << std::endl;
            return {};
        }
    }
    int pool = 0;
    if (rerank) {   // (DIVERSIFIED TOP-N, GROUP CAPS: pool 0 is min(1024, max(topN, 4 topN)), with a cap 8 topN)
        pool = q.pool ? q.pool : std::min(MI355REC_MAX_TOPN_FAST, std::max(topN, (capped ? 8 : 4) * std::min(topN, MI355REC_MAX_TOPN_FAST)));
        if (pool < 0) {
            std::cerr << "Error: pool must be positive (or 0 for the default)" << std::endl;
            return {};
        }
    }
    if (q.maxPerArtist < 0) {
        std::cerr << "Error: maxPerArtist must be positive" << std::endl;
        return {};
    }
    if (capped && !ensureGroups(impl)) return {};
    if (withPrior && !ensurePriors(impl)) return {};
    if (!q.genreIds.empty() && !ensureGenres(impl)) return {};
    impl->idxBuf.assign(static_cast<size_t>(topN), -1);
    impl->scoreBuf.assign(static_cast<size_t>(topN), 0.0f);
    int count = 0;
    const auto shared = [&](auto& r) {   // what mi355rec_playlist_query_t and mi355rec_distance_query_t have in common
        r.size = sizeof r;
        r.rows = rows.data();
        r.k = static_cast<int32_t>(rows.size());
        r.exclude_global = excl.data();
        r.n_exclude = static_cast<int32_t>(excl.size());
        r.filter = q.where.empty() ? nullptr : &f;
        if (!q.genreIds.empty()) {
            r.labels = q.genreIds.data();
            r.n_labels = static_cast<int32_t>(q.genreIds.size());
        }
        r.topn = topN;
    };
    // (an ext whose two pointers are null is the plain request, and a request without flags the plain playlist call: the launches
    // are those of the legacy entry points)
    const mi355rec_request_ext_t ext = requestExt(impl, q.scales.empty() ? nullptr : q.scales.data());
    int rc;
    std::vector<int32_t> member;
    int64_t matching = -1;
    if (q.bounded) {
        mi355rec_bounded_query_t b{};
        shared(b);
        b.metric = q.euclidean ? MI355REC_BOUNDED_EUCLIDEAN : MI355REC_BOUNDED_COSINE;
        b.bound = q.bound;
        mi355rec_bounded_result_t res{};
        res.out_idx = impl->idxBuf.data();
        res.out_score = impl->scoreBuf.data();
        res.out_count = &count;
        res.out_total = &matching;
        rc = mi355rec_sharded_query_bounded_request(impl->engine, &b, &ext, &res);
    } else if (q.jaccard) {
        mi355rec_jaccard_query_t j{};
        shared(j);
        mi355rec_jaccard_result_t res{};
        res.out_idx = impl->idxBuf.data();
        res.out_similarity = impl->scoreBuf.data();
        res.out_count = &count;
        rc = mi355rec_sharded_query_jaccard_request(impl->engine, &j, &ext, &res);
    } else if (q.manhattan) {
        mi355rec_manhattan_query_t m{};
        shared(m);
        mi355rec_manhattan_result_t res{};
        res.out_idx = impl->idxBuf.data();
        res.out_distance = impl->scoreBuf.data();
        res.out_count = &count;
        rc = mi355rec_sharded_query_manhattan_request(impl->engine, &m, &ext, &res);
    } else if (q.anyOf) {
        mi355rec_anyof_query_t a{};
        shared(a);
        member.assign(static_cast<size_t>(topN), -1);
        mi355rec_anyof_result_t res{};
        res.out_idx = impl->idxBuf.data();
        res.out_score = impl->scoreBuf.data();
        res.out_member = member.data();
        res.out_count = &count;
        rc = mi355rec_sharded_query_anyof_request(impl->engine, &a, &ext, &res);
    } else if (q.euclidean) {
        mi355rec_distance_query_t d{};
        shared(d);
        mi355rec_distance_result_t res{};
        res.out_idx = impl->idxBuf.data();
        res.out_distance = impl->scoreBuf.data();
        res.out_count = &count;
        rc = score ? mi355rec_sharded_score_distance_request_candidates(impl->engine, &d, &ext, score->songs.data(),
                                                                        static_cast<int64_t>(score->songs.size()), score->values.data(),
                                                                        score->admissible.data())
             : impl->hasCandidates ? mi355rec_sharded_query_distance_request_candidates(impl->engine, &d, &ext, impl->candidates.data(),
                                                                                       static_cast<int64_t>(impl->candidates.size()), &res)
                                   : mi355rec_sharded_query_distance_request_ext(impl->engine, &d, &ext, &res);
    } else {
        mi355rec_playlist_query_t p{};
        shared(p);
        p.flags = (rerank ? MI355REC_PQ_DIVERSE : 0u) | (capped ? MI355REC_PQ_CAPPED : 0u) | (withPrior ? MI355REC_PQ_PRIOR : 0u);
        p.weights = q.weights.empty() ? nullptr : q.weights.data();
        p.prior_weight = q.priorWeight;
        if (rerank) {
            p.lambda = q.lambda;
            p.pool = pool;
            p.max_per_group = q.maxPerArtist;
        }
        mi355rec_playlist_result_t res{};
        res.out_idx = impl->idxBuf.data();
        res.out_score = impl->scoreBuf.data();
        res.out_count = &count;
        rc = score ? mi355rec_sharded_score_playlist_request_candidates(impl->engine, &p, &ext, score->songs.data(),
                                                                        static_cast<int64_t>(score->songs.size()), score->values.data(),
                                                                        score->admissible.data())
             : impl->hasCandidates ? mi355rec_sharded_query_playlist_request_candidates(impl->engine, &p, &ext, impl->candidates.data(),
                                                                                       static_cast<int64_t>(impl->candidates.size()), &res)
                                   : mi355rec_sharded_query_playlist_request_ext(impl->engine, &p, &ext, &res);
    }
    if (rc != MI355REC_OK) {
        std::cerr << "Error: " << mi355rec_sharded_last_error(impl->engine) << std::endl;
        return {};
    }
    if (score) {
        score->ok = true;
        return {};
    }
    std::vector<int> results(static_cast<size_t>(count));
    for (int i = 0; i < count; ++i) results[i] = static_cast<int>(impl->idxBuf[i]);
    impl->lastScores.assign(impl->scoreBuf.begin(), impl->scoreBuf.begin() + count);
    impl->lastMatchCount = matching;
    if (q.anyOf)
        for (int i = 0; i < count; ++i) impl->lastMatched.push_back(q.songs[static_cast<size_t>(member[static_cast<size_t>(i)])]);
    return results;
}

// What every recommendForPlaylist overload starts its Query from.
Recommender::Query playlistOf(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                              const std::vector<Recommender::FeatureRange>& where, const std::vector<int>& alsoExclude) {
    Recommender::Query q;
    q.songs = songIndices;
    q.topN = topN;
    q.weights = weights;
    q.where = where;
    q.alsoExclude = alsoExclude;
    return q;
}

}  // namespace

std::vector<int> Recommender::recommendQuery(const Query& query) { return runQuery(impl_, query, false); }

std::vector<float> Recommender::scoreSongs(const Query& query, const std::vector<int64_t>& songIndices, std::vector<char>* admissible) {
    if (admissible) admissible->clear();
    for (int64_t i : songIndices)
        if (impl_->initialized && (i < 0 || i >= impl_->numSongs)) {
            std::cerr << "Error: Invalid song index: " << i << std::endl;
            return {};
        }
    ScoreSongs score{songIndices, std::vector<float>(songIndices.size()), std::vector<uint8_t>(songIndices.size())};
    runQuery(impl_, query, false, &score);
    if (!score.ok) return {};
    if (admissible) admissible->assign(score.admissible.begin(), score.admissible.end());
    return score.values;
}

std::vector<int> Recommender::recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<int>& alsoExclude) {
    return recommendQuery(playlistOf(songIndices, topN, {}, {}, alsoExclude));
}

std::vector<int> Recommender::recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<FeatureRange>& where,
                                                   const std::vector<int>& alsoExclude) {
    return recommendQuery(playlistOf(songIndices, topN, {}, where, alsoExclude));
}

std::vector<int> Recommender::recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                                                   const std::vector<FeatureRange>& where, const std::vector<int>& alsoExclude) {
    if (weights.size() != songIndices.size()) {   // (this overload alone takes no empty weight list)
        std::cerr << "Error: " << weights.size() << " weights for " << songIndices.size() << " songs (one weight per song)" << std::endl;
        return {};
    }
    return recommendQuery(playlistOf(songIndices, topN, weights, where, alsoExclude));
}

std::vector<int> Recommender::recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                                                   const std::vector<FeatureRange>& where, const std::vector<int>& alsoExclude, float lambda,
                                                   int pool) {
    Query q = playlistOf(songIndices, topN, weights, where, alsoExclude);
    q.diverse = true;
    q.lambda = lambda;
    q.pool = pool;
    return recommendQuery(q);
}

std::vector<int> Recommender::recommendForPlaylist(const std::vector<int>& songIndices, int topN, const std::vector<float>& weights,
                                                   const std::vector<FeatureRange>& where, const std::vector<int>& alsoExclude, float lambda,
                                                   int pool, int maxPerArtist, const std::vector<int>& genreIds, float priorWeight) {
    // Within genres (or with a prior weight) maxPerArtist 0 asks for no cap: the diversified call (with lambda 1 the plain
    // request: runQuery).  Without either it is refused like every other value below 1.
    const bool wholeFamily = !genreIds.empty() || priorWeight != 0.0f;
    Query q = playlistOf(songIndices, topN, weights, where, alsoExclude);
    q.diverse = true;
    q.lambda = lambda;
    q.pool = pool;
    q.maxPerArtist = maxPerArtist == 0 && !wholeFamily ? -1 : maxPerArtist;
    q.genreIds = genreIds;
    q.priorWeight = priorWeight;
    return recommendQuery(q);
}

std::vector<int> Recommender::recommendNearest(const std::vector<int>& songIndices, int topN, const std::vector<FeatureRange>& where,
                                               const std::vector<int>& genreIds) {
    return recommendScaled(songIndices, topN, {}, true, where, genreIds);
}

std::vector<int> Recommender::recommendScaled(const std::vector<int>& songIndices, int topN, const std::vector<float>& scales, bool euclidean,
                                              const std::vector<FeatureRange>& where, const std::vector<int>& genreIds) {
    Query q = playlistOf(songIndices, topN, {}, where, {});
    q.genreIds = genreIds;
    q.scales = scales;
    q.euclidean = euclidean;
    return runQuery(impl_, q, /*rangesLast=*/true);
}

std::vector<int> Recommender::recommendByIndexCapped(int songIndex, int topN, int maxPerArtist, float lambda, int pool,
                                                     const std::vector<FeatureRange>& where) {
    if (!checkQuery(impl_, songIndex, topN)) return {};
    return recommendForPlaylist({songIndex}, topN, {}, where, {}, lambda, pool, maxPerArtist);
}

std::vector<int> Recommender::recommendDiverse(int songIndex, int topN, float lambda, int pool, const std::vector<FeatureRange>& where) {
    if (!checkQuery(impl_, songIndex, topN)) return {};
    return recommendForPlaylist({songIndex}, topN, {}, where, {}, lambda, pool);
}

std::vector<int> Recommender::recommendForTaste(const std::vector<int>& liked, const std::vector<int>& disliked, int topN,
                                                float dislikeWeight, const std::vector<FeatureRange>& where,
                                                const std::vector<int>& alsoExclude) {
    if (liked.empty()) {
        std::cerr << "Error: at least one liked song is needed" << std::endl;
        return {};
    }
    if (!(dislikeWeight >= 0.0f)) {   // (NaN too)
        std::cerr << "Error: dislikeWeight must be >= 0" << std::endl;
        return {};
    }
    std::vector<int> songs(liked);
    songs.insert(songs.end(), disliked.begin(), disliked.end());
    std::vector<float> weights(liked.size(), 1.0f);
    weights.insert(weights.end(), disliked.size(), -dislikeWeight);
    return recommendForPlaylist(songs, topN, weights, where, alsoExclude);
}

std::vector<int> Recommender::recommendByIndexWhere(int songIndex, int topN, const std::vector<FeatureRange>& where) {
    if (!checkQuery(impl_, songIndex, topN)) return {};
    return recommendForPlaylist({songIndex}, topN, where, {});
}

std::vector<int> Recommender::recommend(const std::string& trackId, int topN) {  // :356-363
    const auto it = impl_->byId.find(trackId);
    if (it == impl_->byId.end()) {
        std::cerr << "Error: Song with track_id '" << trackId << "' not found" << std::endl;
        return {};
    }
    return recommendByIndex(it->second, topN);
}

std::vector<int> Recommender::recommendByName(const std::string& trackName, int topN) {  // :365-372
    const std::string needle = toLower(trackName);
    int index = -1;
    for (size_t i = 0; i < impl_->lowerNames.size(); ++i) {  // exact pass, :340-344
        if (impl_->lowerNames[i] == needle) {
            index = static_cast<int>(i);
            break;
        }
    }
    if (index < 0) {
        for (size_t i = 0; i < impl_->lowerNames.size(); ++i) {  // substring pass, :347-351
            if (impl_->lowerNames[i].find(needle) != std::string::npos) {
                index = static_cast<int>(i);
                break;
            }
        }
    }
    if (index < 0) {
        std::cerr << "Error: Song with name '" << trackName << "' not found" << std::endl;
        return {};
    }
    return recommendByIndex(index, topN);
}

bool Recommender::isInitialized() const { return impl_->initialized; }
bool Recommender::isGPUEnabled() const { return impl_->gpuEnabled; }
int Recommender::getSongCount() const { return impl_->numSongs; }

const std::vector<float>& Recommender::lastScores() const { return impl_->lastScores; }
const std::vector<int>& Recommender::lastMatchedSongs() const { return impl_->lastMatched; }
long long Recommender::lastMatchCount() const { return impl_->lastMatchCount; }

bool Recommender::similarities(int songIndex, std::vector<float>& out) {  // Recommender.cu:184-254
    if (!impl_->initialized || songIndex < 0 || songIndex >= impl_->numSongs) {
        std::cerr << "Error: Invalid query index or recommender not initialized" << std::endl;
        return false;
    }
    out.resize(static_cast<size_t>(impl_->numSongs));
    return mi355rec_sharded_scores_row(impl_->engine, songIndex, out.data()) == MI355REC_OK;
}
