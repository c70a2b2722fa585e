// main.cpp — the drop-in CLI: the reference's three modes (main.cpp:133-189)
// over the MI355X engine.  Written against include/Recommender.h /
// DataManager.h / Song.h only, exactly as the reference's main.cpp is written
// against its own headers — the reference's main.cpp compiles against these
// headers unchanged; this file exists so the repo is self-contained.
//
//   recommender --preprocess <csv>
//   recommender --song "<name>" [-n N]
//   recommender --id "<track_id>" [-n N]
//   ... either query mode with one or more --genre NAME: recommendations only from those genres (extension)
//   recommender --playlist "<track_id>,<track_id>,..." [-n N]: what goes with a playlist of up to 32 songs (extension)
//   ... --playlist with one or more --genre NAME: only songs of those genres, together with any of --where, --dislike,
//       --weights, --diverse, --pool and --max-per-artist (extension); for one song, --playlist <one id> --genre ...
//   ... --song, --id and --playlist with one or more --where NAME=LO:HI: only songs whose feature NAME lies in [LO, HI]
//       (normalised units; extension; with --genre in the --playlist mode only)
//   ... --song, --id and --playlist with --diverse LAMBDA [--pool P]: diversified results (maximal marginal relevance over the
//       P most similar songs; extension; usable with --where, --dislike, --weights; with --genre in the --playlist mode only)
//   ... --song, --id and --playlist with --max-per-artist M: at most M results per primary artist (extension; combines with
//       --where, --dislike, --weights, --diverse and --pool; with --genre in the --playlist mode only)
//   ... --playlist with --priors FILE --prior-weight BETA: rank by similarity + BETA x prior (extension; FILE holds one float in
//       [-1, 1] per line, in catalogue order; usable with every other option of the --playlist mode)
//   ... --song, --id and --playlist with --metric euclidean: the NEAREST songs by Euclidean distance over the 12 features instead
//       of the most similar by cosine (extension; with --genre and --where; distances are printed)
//   ... --song, --id and --playlist with one or more --scale NAME=S: feature NAME counts S times (0: ignored) in the similarity or
//       the distance (extension; under both metrics, with --genre and --where)
//   ... --song, --id and --playlist with --seen FILE or --only FILE (track ids, one per line): the listed songs are never recommended
//       (--seen: a listening history of any length) or only the listed songs are ranked (--only: a candidate set); extension, beside
//       every other option of those modes; --song / --id then run as the one-song playlist (not with --genre there)
//   ... --playlist with --dislike "<track_id>,..." [--dislike-weight W] [--weights "w,w,..."]: weighted playlists (extension):
//       the disliked songs push results away (weight -W, default 0.5), --weights gives the playlist's songs their own weights
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "DataManager.h"
#include "Recommender.h"
#include "Song.h"

static const std::string kBinaryDataFile = "songs_data.bin";  // main.cpp:11

static void usage(const char* prog) {
    std::cout << "Music Recommendation Engine - Usage:\n\n"
              << "1. Preprocessing Mode:\n   " << prog << " --preprocess <path_to_csv>\n"
              << "   Processes CSV file and creates binary data file.\n\n"
              << "2. Recommendation Mode (by song name):\n   " << prog << " --song \"Song Name\" [-n N]\n"
              << "   Returns top N similar songs (default N=10).\n\n"
              << "3. Recommendation Mode (by track ID):\n   " << prog << " --id \"track_id\" [-n N]\n"
              << "   Returns top N similar songs (default N=10).\n\n"
              << "Filter (extension): --where NAME=LO:HI, repeatable, with --song, --id or --playlist (with --genre: --playlist only):\n"
              << "   only songs whose feature NAME lies in [LO, HI].  NAME is a CSV feature column (danceability, energy, key, loudness,\n"
              << "   mode, speechiness, acousticness, instrumentalness, liveness, valence, tempo); LO and HI are in the\n"
              << "   normalised [0, 1] units songs_data.bin holds (min-max over the CSV), not raw BPM or dB.\n\n"
              << "Weighted playlists (extension): " << prog << " --playlist \"id,id,...\" [--dislike \"id,...\"] [--dislike-weight W]\n"
              << "   [--weights \"w,w,...\"]: songs like the playlist's and unlike the disliked ones (each counts -W, default 0.5);\n"
              << "   --weights gives one weight per playlist song (default 1 each).  Usable with --where.\n"
              << "Diversified results (extension): --diverse LAMBDA [--pool P], with --song, --id or --playlist (and --where, --dislike,\n"
              << "   --weights; with --genre: --playlist only): picks from the P most similar songs (default 4 x N, at most 1024), each pick\n"
              << "   weighing similarity (LAMBDA in [0, 1]; 1 = the plain result) against likeness to the songs already picked.\n"
              << "Artist cap (extension): --max-per-artist M, with --song, --id or --playlist (and --where, --dislike, --weights,\n"
              << "   --diverse, --pool; with --genre: --playlist only): at most M results by one primary artist (the artists field up to its\n"
              << "   first ';').  Results come from the P most similar songs (--pool; default 8 x N, at most 1024).\n"
              << "Playlists within genres (extension): " << prog << " --playlist \"id,id,...\" --genre NAME [--genre NAME ...]\n"
              << "   with any of --where, --dislike, --weights, --diverse, --pool, --max-per-artist: only songs of those genres.\n"
              << "   With --song / --id, --genre does not combine with --where, --diverse or --max-per-artist: use\n"
              << "   --playlist <one id> --genre ... for those combinations.\n"
              << "Row priors (extension): " << prog << " --playlist \"id,id,...\" --priors FILE --prior-weight BETA, with any other\n"
              << "   --playlist option: ranks by similarity + BETA x prior (BETA in [-4, 4]; negative demotes).  FILE holds one number in\n"
              << "   [-1, 1] per line, one line per song in the order of songs_data.bin (a popularity column scaled to [0, 1], say).\n"
              << "Euclidean metric (extension): --metric euclidean, with --song, --id or --playlist (and --genre, --where): the nearest\n"
              << "   songs by distance over the 12 normalised features (for a playlist: the root-mean-square distance to its songs).\n"
              << "   Cosine ignores how large the features are; the distance does not.  Not with --diverse, --weights, --dislike,\n"
              << "   --priors or --max-per-artist.  --metric cosine is the default.\n"
              << "Feature scales (extension): --scale NAME=S, repeatable, with --song, --id or --playlist, under both metrics (and\n"
              << "   --genre, --where): every song's feature NAME is multiplied by S (0 to 1024) before songs are compared, so S = 0\n"
              << "   ignores the feature and S = 2 makes it count double; features not named keep 1.  NAME is one of --where's names or\n"
              << "   genre (the numeric genre id).  --where still tests the stored values.  Not with --diverse, --pool,\n"
              << "   --max-per-artist, --priors, --weights or --dislike.\n"
              << "Row sets (extension): --seen FILE or --only FILE (not both), with --song, --id or --playlist and every other option of\n"
              << "   those modes: FILE holds track ids, one per line.  --seen: those songs are never recommended (a listening history, of\n"
              << "   any length).  --only: only those songs are ranked (a candidate set).  Lines that name no song of the catalogue are\n"
              << "   skipped and counted.  With --song / --id (the one-song playlist) not together with --genre: use --playlist <one id>.\n"
              << std::endl;
}

// --where NAME=LO:HI, any number of times from argv[first]: the ranges (feature indices in Song.h order).  false, with a
// message, on a malformed option or an unknown NAME.
static bool parseWhere(int argc, char* argv[], int first, std::vector<Recommender::FeatureRange>& ranges) {
    static const char* const kNames[] = {"danceability", "energy", "key", "loudness", "mode", "speechiness",
                                         "acousticness", "instrumentalness", "liveness", "valence", "tempo"};
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--where") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --where needs NAME=LO:HI" << std::endl;
            return false;
        }
        const std::string arg = argv[++i];
        const size_t eq = arg.find('='), colon = arg.find(':', eq == std::string::npos ? 0 : eq);
        if (eq == std::string::npos || colon == std::string::npos) {
            std::cerr << "Error: --where '" << arg << "': expected NAME=LO:HI" << std::endl;
            return false;
        }
        const std::string name = arg.substr(0, eq), lo = arg.substr(eq + 1, colon - eq - 1), hi = arg.substr(colon + 1);
        int feature = -1;
        for (int j = 0; j < 11; ++j)
            if (name == kNames[j]) feature = j;
        if (feature < 0) {
            std::cerr << "Error: --where: unknown feature '" << name << "'" << std::endl;
            return false;
        }
        char* end1 = nullptr;
        char* end2 = nullptr;
        const float l = std::strtof(lo.c_str(), &end1), h = std::strtof(hi.c_str(), &end2);
        if (lo.empty() || hi.empty() || *end1 != '\0' || *end2 != '\0') {
            std::cerr << "Error: --where '" << arg << "': LO and HI must be numbers" << std::endl;
            return false;
        }
        ranges.push_back({feature, l, h});
    }
    return true;
}

// --scale NAME=S, any number of times from argv[first]: scales = 12 factors in Song.h order (1 where not named), or empty when the
// option is not given.  false, with a message, on a malformed option, an unknown NAME or an option --scale is not served with.
static bool parseScale(int argc, char* argv[], int first, std::vector<float>& scales) {
    static const char* const kNames[] = {"danceability", "energy", "key", "loudness", "mode", "speechiness",
                                         "acousticness", "instrumentalness", "liveness", "valence", "tempo", "genre"};
    scales.clear();
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--scale") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --scale needs NAME=S" << std::endl;
            return false;
        }
        const std::string arg = argv[++i];
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) {
            std::cerr << "Error: --scale '" << arg << "': expected NAME=S" << std::endl;
            return false;
        }
        const std::string name = arg.substr(0, eq), value = arg.substr(eq + 1);
        int feature = -1;
        for (int j = 0; j < 12; ++j)
            if (name == kNames[j]) feature = j;
        if (feature < 0) {
            std::cerr << "Error: --scale: unknown feature '" << name << "'" << std::endl;
            return false;
        }
        char* end = nullptr;
        const float v = std::strtof(value.c_str(), &end);
        if (value.empty() || *end != '\0') {
            std::cerr << "Error: --scale '" << arg << "': S must be a number" << std::endl;
            return false;
        }
        if (scales.empty()) scales.assign(12, 1.0f);
        scales[static_cast<size_t>(feature)] = v;
    }
    if (scales.empty()) return true;
    for (int i = first; i < argc; ++i)
        for (const char* no : {"--diverse", "--pool", "--weights", "--dislike", "--dislike-weight", "--priors", "--prior-weight", "--max-per-artist"})
            if (std::strcmp(argv[i], no) == 0) {
                std::cerr << "Error: --scale cannot be combined with " << no << " (scaled requests take --metric, --genre and --where only)"
                          << std::endl;
                return false;
            }
    std::cout << "Feature scales:";
    for (int j = 0; j < 12; ++j)
        if (scales[static_cast<size_t>(j)] != 1.0f) std::cout << " " << kNames[j] << "=" << scales[static_cast<size_t>(j)];
    std::cout << std::endl;
    return true;
}

static bool preprocessMode(const std::string& csvPath) {  // main.cpp:33-44
    std::cout << "=== PREPROCESSING MODE ===" << std::endl;
    if (!DataManager::preprocessData(csvPath, kBinaryDataFile)) {
        std::cerr << "Preprocessing failed!" << std::endl;
        return false;
    }
    std::cout << "\nPreprocessing successful!\nBinary data saved to: " << kBinaryDataFile << std::endl;
    return true;
}

static void printSong(const Song& s, std::map<int, std::string>& genres, const char* indent) {
    std::cout << indent << "Artist: " << s.artists << "\n"
              << indent << "Genre:  " << genres[s.genre_id] << "\n"
              << indent << "ID:     " << s.track_id << std::endl;
}

// --diverse LAMBDA [--pool P] (diversified results).
struct DiverseOpt {
    bool on = false;
    float lambda = 1.0f;
    int pool = 0;   // 0: the default, min(1024, 4 x N)
    int maxPerArtist = 0;   // --max-per-artist M (0: not given); the default pool is then min(1024, 8 x N)
};

// false, with a message, on a malformed or out-of-range option.
static bool parseDiverse(int argc, char* argv[], int first, int topN, DiverseOpt& dv) {
    bool havePool = false;
    for (int i = first; i < argc; ++i) {
        const bool diverse = std::strcmp(argv[i], "--diverse") == 0, pool = std::strcmp(argv[i], "--pool") == 0,
                   cap = std::strcmp(argv[i], "--max-per-artist") == 0;
        if (!diverse && !pool && !cap) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: " << argv[i] << " needs a value" << std::endl;
            return false;
        }
        const std::string arg = argv[++i];
        char* end = nullptr;
        if (diverse) {
            dv.on = true;
            dv.lambda = std::strtof(arg.c_str(), &end);
            if (arg.empty() || *end != '\0' || !(dv.lambda >= 0.0f && dv.lambda <= 1.0f)) {   // (NaN too)
                std::cerr << "Error: --diverse '" << arg << "': LAMBDA must be a number in [0, 1]" << std::endl;
                return false;
            }
        } else if (cap) {
            const long v = std::strtol(arg.c_str(), &end, 10);
            if (arg.empty() || *end != '\0' || v < 1 || v > 1024) {
                std::cerr << "Error: --max-per-artist '" << arg << "': M must be an integer in [1, " << 1024 << "]" << std::endl;
                return false;
            }
            dv.maxPerArtist = static_cast<int>(v);
        } else {
            havePool = true;
            const long v = std::strtol(arg.c_str(), &end, 10);
            if (arg.empty() || *end != '\0' || v < 1 || v > 1024) {
                std::cerr << "Error: --pool '" << arg << "': P must be an integer in [1, " << 1024 << "]" << std::endl;
                return false;
            }
            dv.pool = static_cast<int>(v);
        }
    }
    if (dv.maxPerArtist > 0) dv.on = true;   // (without --diverse: lambda 1, the plain order with the cap)
    if (havePool && !dv.on) {
        std::cerr << "Error: --pool needs --diverse LAMBDA or --max-per-artist M" << std::endl;
        return false;
    }
    if (havePool && dv.pool < topN) {
        std::cerr << "Error: --pool " << dv.pool << " is below -n " << topN << " (picks are made from the pool)" << std::endl;
        return false;
    }
    return true;
}

// --seen FILE / --only FILE from argv[first] (row sets): what main() found, for the modes below.
struct RowSetOpt {
    bool on = false, only = false;
    std::string file;
};
static RowSetOpt g_rowSet;

static bool parseRowSet(int argc, char* argv[], int first, RowSetOpt& rs) {
    for (int i = first; i < argc; ++i) {
        const bool seen = std::strcmp(argv[i], "--seen") == 0, only = std::strcmp(argv[i], "--only") == 0;
        if (!seen && !only) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: " << argv[i] << " needs a file of track ids (one per line)" << std::endl;
            return false;
        }
        if (rs.on) {
            std::cerr << "Error: --seen and --only cannot be combined, and each is given once (a request takes one row set)" << std::endl;
            return false;
        }
        rs.on = true;
        rs.only = only;
        rs.file = argv[++i];
    }
    return true;
}

// The reference loads every Song, deep-copies the vector into the recommender and
// flattens it again (main.cpp:50-60, Recommender.cu:109,162-167).  Here the file is
// walked once (DataManager::loadCatalogue): the feature matrix goes to the engine as
// it is, and only the handful of songs that are PRINTED are read back in full.
static std::string lowered(std::string s) {
    std::transform(s.begin(), s.end(), s.begin(), ::tolower);
    return s;
}

// The query song's row by the engine's rules (exact id / exact name, then substring); -1 if none.
static int findQuery(const DataManager::Catalogue& catalogue, const std::string& query, bool isTrackId) {
    int index = -1;
    if (isTrackId) {
        for (size_t i = 0; i < catalogue.size() && index < 0; ++i)
            if (catalogue.trackIds[i] == query) index = static_cast<int>(i);
    } else {
        const std::string needle = lowered(query);
        for (size_t i = 0; i < catalogue.size() && index < 0; ++i)
            if (lowered(catalogue.trackNames[i]) == needle) index = static_cast<int>(i);
        for (size_t i = 0; i < catalogue.size() && index < 0; ++i)
            if (lowered(catalogue.trackNames[i]).find(needle) != std::string::npos) index = static_cast<int>(i);
    }
    return index;
}

// --seen / --only: the file's track ids (one per line, blank lines skipped, the first row of an id as for --id) to the recommender
// as its row set.  A line that names no song of the catalogue is skipped; how many were is said on stderr (a history normally
// holds tracks the catalogue lacks).  false, with a message, when the file cannot be read or the set is refused.
static bool applyRowSet(Recommender& recommender, const DataManager::Catalogue& catalogue) {
    if (!g_rowSet.on) return true;
    std::ifstream in(g_rowSet.file);
    if (!in) {
        std::cerr << "Error: cannot open the row set file '" << g_rowSet.file << "'" << std::endl;
        return false;
    }
    std::unordered_map<std::string, int> byId;
    for (size_t i = 0; i < catalogue.size(); ++i) byId.emplace(catalogue.trackIds[i], static_cast<int>(i));   // (the first row of an id)
    std::vector<int> rows;
    size_t skipped = 0;
    std::string line;
    while (std::getline(in, line)) {
        const size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        const auto hit = byId.find(line.substr(a, line.find_last_not_of(" \t\r") - a + 1));
        if (hit == byId.end()) ++skipped;
        else rows.push_back(hit->second);
    }
    std::cerr << "Row set (" << (g_rowSet.only ? "--only" : "--seen") << " " << g_rowSet.file << "): " << rows.size() << " tracks, " << skipped
              << " lines skipped (not in the catalogue)" << std::endl;
    if (!recommender.setRowSet(rows, g_rowSet.only)) return false;
    std::cout << (g_rowSet.only ? "Only among " : "Leaving out ") << rows.size() << " listed songs" << std::endl;
    return true;
}

// --where: the songs within every range, ranked as recommendByIndex ranks the whole catalogue.
static void whereRecommendations(Recommender& recommender, const DataManager::Catalogue& catalogue, const std::string& query,
                                 bool isTrackId, int topN, const std::vector<Recommender::FeatureRange>& ranges, std::vector<int>& recs) {
    const int index = findQuery(catalogue, query, isTrackId);
    if (index < 0) {
        std::cerr << "Error: Song with " << (isTrackId ? "track_id" : "name") << " '" << query << "' not found" << std::endl;
        return;   // (no recommendations: the caller says so)
    }
    recs = recommender.recommendByIndexWhere(index, topN, ranges);
}

// The ids of the genres named (case-insensitively); false, with a message, for an unknown one.
static bool genreIdsOf(const DataManager::Catalogue& catalogue, const std::vector<std::string>& genres, std::vector<int>& ids) {
    for (const std::string& name : genres) {
        int id = -1;
        for (const auto& g : catalogue.genreMap)
            if (lowered(g.second) == lowered(name)) { id = g.first; break; }
        if (id < 0) {
            std::cerr << "Error: Unknown genre '" << name << "'" << std::endl;
            return false;
        }
        ids.push_back(id);
    }
    return true;
}

// --genre: the songs whose genre is one of `genres` (names matched case-insensitively), ranked as recommendByIndex
// ranks the whole catalogue; the query song is found by the engine's rules (exact id / exact name, then substring).
static bool genreRecommendations(Recommender& recommender, const DataManager::Catalogue& catalogue, const std::string& query,
                                 bool isTrackId, int topN, const std::vector<std::string>& genres, std::vector<int>& recs) {
    std::vector<int> ids;
    if (!genreIdsOf(catalogue, genres, ids)) return false;
    const int index = findQuery(catalogue, query, isTrackId);
    if (index < 0) {
        std::cerr << "Error: Song with " << (isTrackId ? "track_id" : "name") << " '" << query << "' not found" << std::endl;
        return true;   // (no recommendations: the caller says so)
    }
    std::cout << "Restricted to genres:";
    for (const std::string& name : genres) std::cout << " " << name;
    std::cout << std::endl;
    if (!recommender.setGenreIds(catalogue.genreIds)) return true;
    recs = recommender.recommendByIndexInGenres(index, topN, ids);
    return true;
}

// --max-per-artist: the group ids of the catalogue's songs (their primary artists, read back from the file) to the recommender.
static bool capByArtist(Recommender& recommender, const DataManager::Catalogue& catalogue) {
    std::vector<std::string> artists(catalogue.size());
    Song song;
    for (size_t i = 0; i < catalogue.size(); ++i) {
        if (!DataManager::readSong(catalogue, i, song)) {
            std::cerr << "Error: could not read song " << i << " from " << catalogue.path << std::endl;
            return false;
        }
        artists[i] = song.artists;
    }
    return recommender.setGroupIds(Recommender::artistGroupIds(artists));
}

// --diverse: recommendByIndex (or its --where form) diversified.
static void diverseRecommendations(Recommender& recommender, const DataManager::Catalogue& catalogue, const std::string& query,
                                   bool isTrackId, int topN, const std::vector<Recommender::FeatureRange>& ranges, const DiverseOpt& dv,
                                   std::vector<int>& recs) {
    const int index = findQuery(catalogue, query, isTrackId);
    if (index < 0) {
        std::cerr << "Error: Song with " << (isTrackId ? "track_id" : "name") << " '" << query << "' not found" << std::endl;
        return;   // (no recommendations: the caller says so)
    }
    if (dv.maxPerArtist > 0) {
        if (!capByArtist(recommender, catalogue)) return;
        std::cout << "At most " << dv.maxPerArtist << " per artist";
        if (dv.lambda < 1.0f) std::cout << "; diversified: lambda " << dv.lambda;
        std::cout << std::endl;
        recs = recommender.recommendByIndexCapped(index, topN, dv.maxPerArtist, dv.lambda, dv.pool, ranges);
        return;
    }
    std::cout << "Diversified: lambda " << dv.lambda << std::endl;
    recs = recommender.recommendDiverse(index, topN, dv.lambda, dv.pool, ranges);
}

static bool recommendationMode(const std::string& query, bool isTrackId, int topN, const std::vector<std::string>& genres,
                               const std::vector<Recommender::FeatureRange>& ranges, const DiverseOpt& dv) {  // main.cpp:46-131
    std::cout << "=== RECOMMENDATION MODE ===" << std::endl;
    DataManager::Catalogue catalogue;
    if (!DataManager::loadCatalogue(kBinaryDataFile, catalogue)) {
        std::cerr << "Failed to load data. Have you run preprocessing?" << std::endl;
        return false;
    }
    Recommender recommender;
    if (!recommender.initialize(catalogue.features, catalogue.trackIds, catalogue.trackNames)) {
        std::cerr << "Failed to initialize recommender" << std::endl;
        return false;
    }
    if (!applyRowSet(recommender, catalogue)) return false;
    std::map<int, std::string>& genreMap = catalogue.genreMap;

    std::vector<int> recs;
    int queryIndex = -1;
    if (isTrackId) {
        std::cout << "\nSearching for track ID: " << query << std::endl;
        if (dv.on) diverseRecommendations(recommender, catalogue, query, true, topN, ranges, dv, recs);
        else if (!ranges.empty() || g_rowSet.on) whereRecommendations(recommender, catalogue, query, true, topN, ranges, recs);   // (a row set: the one-song playlist)
        else if (genres.empty()) recs = recommender.recommend(query, topN);
        else if (!genreRecommendations(recommender, catalogue, query, true, topN, genres, recs)) return false;
        for (size_t i = 0; i < catalogue.size(); ++i)
            if (catalogue.trackIds[i] == query) { queryIndex = static_cast<int>(i); break; }
    } else {
        std::cout << "\nSearching for song: " << query << std::endl;
        if (dv.on) diverseRecommendations(recommender, catalogue, query, false, topN, ranges, dv, recs);
        else if (!ranges.empty() || g_rowSet.on) whereRecommendations(recommender, catalogue, query, false, topN, ranges, recs);
        else if (genres.empty()) recs = recommender.recommendByName(query, topN);
        else if (!genreRecommendations(recommender, catalogue, query, false, topN, genres, recs)) return false;
        // The reference finds the song it DISPLAYS with a single exact-or-substring
        // pass (main.cpp:85-95), not the engine's exact-then-substring rule; kept.
        std::string needle = query;
        std::transform(needle.begin(), needle.end(), needle.begin(), ::tolower);
        for (size_t i = 0; i < catalogue.size(); ++i) {
            std::string name = catalogue.trackNames[i];
            std::transform(name.begin(), name.end(), name.begin(), ::tolower);
            if (name == needle || name.find(needle) != std::string::npos) { queryIndex = static_cast<int>(i); break; }
        }
    }
    if (recs.empty()) {
        std::cerr << "No recommendations found. Please check the query." << std::endl;
        return false;
    }
    Song song;
    if (queryIndex >= 0 && DataManager::readSong(catalogue, static_cast<size_t>(queryIndex), song)) {
        std::cout << "\n----------------------------------------------\nQuery Song:\n"
                  << "  Title:   " << song.track_name << "\n"
                  << "  Artist:  " << song.artists << "\n"
                  << "  Genre:   " << genreMap[song.genre_id] << "\n"
                  << "  ID:      " << song.track_id
                  << "\n----------------------------------------------" << std::endl;
    }
    std::cout << "\nTop " << recs.size() << " Recommendations:\n" << std::endl;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (!DataManager::readSong(catalogue, static_cast<size_t>(recs[i]), song)) {
            std::cerr << "Error: could not read song " << recs[i] << " from " << catalogue.path << std::endl;
            return false;
        }
        std::cout << (i + 1) << ". \"" << song.track_name << "\"" << std::endl;
        printSong(song, genreMap, "   ");
        if (i + 1 < recs.size()) std::cout << std::endl;
    }
    std::cout << "\nRecommendation complete!" << std::endl;
    return true;
}

// --playlist: the songs most similar on average to the playlist's (exact track ids, the first row of an id as for --id),
// the playlist's own songs never among them.
// The non-empty fields of a comma-separated list.
static std::vector<std::string> splitList(const std::string& list) {
    std::vector<std::string> items;
    for (size_t start = 0; start <= list.size();) {
        size_t end = list.find(',', start);
        if (end == std::string::npos) end = list.size();
        if (end > start) items.push_back(list.substr(start, end - start));
        start = end + 1;
    }
    return items;
}

// --dislike / --dislike-weight / --weights of a --playlist call (weighted playlists).
struct Taste {
    bool weighted = false;            // any of the three options was given
    std::vector<std::string> dislike;
    float dislikeWeight = 0.5f;
    bool haveWeights = false;
    std::vector<float> weights;       // of the playlist's songs
};

// false, with a message, on a malformed option.
static bool parseTaste(int argc, char* argv[], int first, Taste& taste) {
    for (int i = first; i < argc; ++i) {
        const bool dislike = std::strcmp(argv[i], "--dislike") == 0, dw = std::strcmp(argv[i], "--dislike-weight") == 0,
                   weights = std::strcmp(argv[i], "--weights") == 0;
        if (!dislike && !dw && !weights) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: " << argv[i] << " needs a value" << std::endl;
            return false;
        }
        const std::string arg = argv[++i];
        taste.weighted = true;
        if (dislike) {
            for (const std::string& id : splitList(arg)) taste.dislike.push_back(id);
            continue;
        }
        for (const std::string& field : dw ? std::vector<std::string>{arg} : splitList(arg)) {
            char* end = nullptr;
            const float v = std::strtof(field.c_str(), &end);
            if (field.empty() || *end != '\0') {
                std::cerr << "Error: " << argv[i - 1] << " '" << arg << "': not a number: '" << field << "'" << std::endl;
                return false;
            }
            if (dw) taste.dislikeWeight = v;
            else taste.weights.push_back(v);
        }
        if (weights) taste.haveWeights = true;
        if (dw && !(taste.dislikeWeight >= 0.0f)) {
            std::cerr << "Error: --dislike-weight must be >= 0" << std::endl;
            return false;
        }
    }
    return true;
}

// --priors FILE --prior-weight BETA of a --playlist call (row priors).
struct PriorOpt {
    bool on = false;
    std::string file;
    float weight = 0.0f;
};

// false, with a message, on a malformed option or one without the other.
static bool parsePrior(int argc, char* argv[], int first, PriorOpt& pr) {
    bool haveWeight = false;
    for (int i = first; i < argc; ++i) {
        const bool file = std::strcmp(argv[i], "--priors") == 0, weight = std::strcmp(argv[i], "--prior-weight") == 0;
        if (!file && !weight) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: " << argv[i] << " needs a value" << std::endl;
            return false;
        }
        const std::string arg = argv[++i];
        if (file) {
            pr.file = arg;
            continue;
        }
        char* end = nullptr;
        pr.weight = std::strtof(arg.c_str(), &end);
        haveWeight = true;
        if (arg.empty() || *end != '\0' || !(pr.weight >= -4.0f && pr.weight <= 4.0f)) {   // (NaN too)
            std::cerr << "Error: --prior-weight '" << arg << "': BETA must be a number in [-4, 4]" << std::endl;
            return false;
        }
    }
    if (haveWeight != !pr.file.empty()) {
        std::cerr << "Error: --priors FILE and --prior-weight BETA go together" << std::endl;
        return false;
    }
    pr.on = haveWeight;
    return true;
}

// The priors file: one number per line (blank lines skipped), `songs` of them.  false, with a message, otherwise.
static bool readPriors(const std::string& path, size_t songs, std::vector<float>& priors) {
    std::ifstream in(path);
    if (!in) {
        std::cerr << "Error: cannot open the priors file '" << path << "'" << std::endl;
        return false;
    }
    std::string line;
    for (size_t lineNo = 1; std::getline(in, line); ++lineNo) {
        const size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        const std::string field = line.substr(a, line.find_last_not_of(" \t\r") - a + 1);
        char* end = nullptr;
        const float v = std::strtof(field.c_str(), &end);
        if (*end != '\0') {
            std::cerr << "Error: " << path << " line " << lineNo << ": not a number: '" << field << "'" << std::endl;
            return false;
        }
        priors.push_back(v);
    }
    if (priors.size() != songs) {
        std::cerr << "Error: " << path << " holds " << priors.size() << " priors for " << songs << " songs (one per line, in catalogue order)"
                  << std::endl;
        return false;
    }
    return true;
}

static bool playlistMode(const std::string& list, int topN, const std::vector<Recommender::FeatureRange>& ranges, const Taste& taste,
                         const DiverseOpt& dv, const std::vector<std::string>& genres, const PriorOpt& pr) {
    std::cout << "=== PLAYLIST MODE ===" << std::endl;
    std::vector<std::string> ids = splitList(list);
    if (ids.empty()) {
        std::cerr << "Error: the playlist names no track" << std::endl;
        return false;
    }
    DataManager::Catalogue catalogue;
    if (!DataManager::loadCatalogue(kBinaryDataFile, catalogue)) {
        std::cerr << "Failed to load data. Have you run preprocessing?" << std::endl;
        return false;
    }
    if (taste.haveWeights && taste.weights.size() != ids.size()) {
        std::cerr << "Error: --weights names " << taste.weights.size() << " weights for " << ids.size() << " playlist songs" << std::endl;
        return false;
    }
    std::vector<int> genreIds;   // --genre: only songs of these genres are recommended (the playlist's own may be of any)
    if (!genreIdsOf(catalogue, genres, genreIds)) return false;
    const size_t liked = ids.size();
    ids.insert(ids.end(), taste.dislike.begin(), taste.dislike.end());
    std::vector<float> weights = taste.haveWeights ? taste.weights : std::vector<float>(liked, 1.0f);
    weights.insert(weights.end(), taste.dislike.size(), -taste.dislikeWeight);
    std::vector<int> members;
    for (const std::string& id : ids) {
        int index = -1;
        for (size_t i = 0; i < catalogue.size() && index < 0; ++i)
            if (catalogue.trackIds[i] == id) index = static_cast<int>(i);
        if (index < 0) {
            std::cerr << "Error: Song with track_id '" << id << "' not found" << std::endl;
            return false;
        }
        members.push_back(index);
    }
    Recommender recommender;
    if (!recommender.initialize(catalogue.features, catalogue.trackIds, catalogue.trackNames)) {
        std::cerr << "Failed to initialize recommender" << std::endl;
        return false;
    }
    if (!applyRowSet(recommender, catalogue)) return false;
    std::map<int, std::string>& genreMap = catalogue.genreMap;
    if (dv.maxPerArtist > 0) {
        if (!capByArtist(recommender, catalogue)) return false;
        std::cout << "At most " << dv.maxPerArtist << " per artist" << std::endl;
    }
    if (dv.on && (dv.maxPerArtist == 0 || dv.lambda < 1.0f)) std::cout << "Diversified: lambda " << dv.lambda << std::endl;
    if (!genreIds.empty()) {
        std::cout << "Restricted to genres:";
        for (const std::string& name : genres) std::cout << " " << name;
        std::cout << std::endl;
        if (!recommender.setGenreIds(catalogue.genreIds)) return false;
    }
    if (pr.on) {
        std::vector<float> priors;
        if (!readPriors(pr.file, catalogue.size(), priors) || !recommender.setPriors(priors)) return false;
        std::cout << "Prior weight: " << pr.weight << " (" << pr.file << ")" << std::endl;
    }
    const bool blended = pr.on && pr.weight != 0.0f;   // (BETA 0 is the call without a prior)
    const std::vector<int> recs = !genreIds.empty() || blended   // (the general overload: lambda 1 without a cap is the plain request)
                                      ? recommender.recommendForPlaylist(members, topN, taste.weighted ? weights : std::vector<float>(), ranges,
                                                                         {}, dv.on ? dv.lambda : 1.0f, dv.on ? dv.pool : 0, dv.maxPerArtist,
                                                                         genreIds, blended ? pr.weight : 0.0f)
                                  : dv.maxPerArtist > 0
                                      ? recommender.recommendForPlaylist(members, topN, taste.weighted ? weights : std::vector<float>(), ranges,
                                                                         {}, dv.lambda, dv.pool, dv.maxPerArtist)
                                  : dv.on         ? recommender.recommendForPlaylist(members, topN, taste.weighted ? weights : std::vector<float>(),
                                                                                     ranges, {}, dv.lambda, dv.pool)
                                  : taste.weighted ? recommender.recommendForPlaylist(members, topN, weights, ranges, {})
                                  : ranges.empty() ? recommender.recommendForPlaylist(members, topN)
                                                   : recommender.recommendForPlaylist(members, topN, ranges, {});
    if (recs.empty()) {
        std::cerr << "No recommendations found. Please check the query." << std::endl;
        return false;
    }
    Song song;
    std::cout << "\n----------------------------------------------\nPlaylist (" << members.size() << " songs):" << std::endl;
    for (size_t i = 0; i < members.size(); ++i) {
        if (!DataManager::readSong(catalogue, static_cast<size_t>(members[i]), song)) {
            std::cerr << "Error: could not read song " << members[i] << " from " << catalogue.path << std::endl;
            return false;
        }
        std::cout << "  " << (i + 1) << ". \"" << song.track_name << "\"";
        if (taste.weighted) std::cout << "  (weight " << weights[i] << ")";
        std::cout << std::endl;
        printSong(song, genreMap, "     ");
    }
    std::cout << "----------------------------------------------" << std::endl;
    std::cout << "\nTop " << recs.size() << " Recommendations:\n" << std::endl;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (!DataManager::readSong(catalogue, static_cast<size_t>(recs[i]), song)) {
            std::cerr << "Error: could not read song " << recs[i] << " from " << catalogue.path << std::endl;
            return false;
        }
        std::cout << (i + 1) << ". \"" << song.track_name << "\"" << std::endl;
        printSong(song, genreMap, "   ");
        if (i + 1 < recs.size()) std::cout << std::endl;
    }
    std::cout << "\nRecommendation complete!" << std::endl;
    return true;
}

// --metric NAME from argv[first]: euclidean = true for "euclidean", false for "cosine" or no option.  false (the return
// value), with a message, for another name, or for euclidean beside an option it is not served with.
static bool parseMetric(int argc, char* argv[], int first, bool& euclidean) {
    euclidean = false;
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--metric") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --metric needs a name (cosine or euclidean)" << std::endl;
            return false;
        }
        const std::string name = argv[++i];
        if (name != "cosine" && name != "euclidean") {
            std::cerr << "Error: --metric '" << name << "': cosine or euclidean" << std::endl;
            return false;
        }
        euclidean = name == "euclidean";
    }
    if (!euclidean) return true;
    for (int i = first; i < argc; ++i)
        for (const char* no : {"--diverse", "--pool", "--weights", "--dislike", "--dislike-weight", "--priors", "--prior-weight", "--max-per-artist"})
            if (std::strcmp(argv[i], no) == 0) {
                std::cerr << "Error: --metric euclidean cannot be combined with " << no
                          << " (distance requests take --genre and --where only)" << std::endl;
                return false;
            }
    return true;
}

// --metric euclidean: the songs nearest to one song (--song / --id) or to a playlist's songs, with their distances; with
// --scale (scales not empty) under either metric: the same over the scaled features, cosine printing its scores.
static bool nearestMode(const std::string& query, bool isPlaylist, bool isTrackId, int topN,
                        const std::vector<Recommender::FeatureRange>& ranges, const std::vector<std::string>& genres,
                        bool euclidean = true, const std::vector<float>& scales = {}) {
    std::cout << (euclidean ? "=== NEAREST MODE (Euclidean distance) ===" : "=== SCALED MODE (cosine over scaled features) ===") << std::endl;
    DataManager::Catalogue catalogue;
    if (!DataManager::loadCatalogue(kBinaryDataFile, catalogue)) {
        std::cerr << "Failed to load data. Have you run preprocessing?" << std::endl;
        return false;
    }
    std::vector<int> genreIds;
    if (!genreIdsOf(catalogue, genres, genreIds)) return false;
    std::vector<int> members;
    const std::vector<std::string> names = isPlaylist ? splitList(query) : std::vector<std::string>{query};
    if (names.empty()) {
        std::cerr << "Error: the playlist names no track" << std::endl;
        return false;
    }
    for (const std::string& name : names) {
        const int index = findQuery(catalogue, name, isPlaylist || isTrackId);
        if (index < 0) {
            std::cerr << "Error: Song with " << (isPlaylist || isTrackId ? "track_id" : "name") << " '" << name << "' not found" << std::endl;
            return false;
        }
        members.push_back(index);
    }
    Recommender recommender;
    if (!recommender.initialize(catalogue.features, catalogue.trackIds, catalogue.trackNames)) {
        std::cerr << "Failed to initialize recommender" << std::endl;
        return false;
    }
    if (!applyRowSet(recommender, catalogue)) return false;
    if (!genreIds.empty()) {
        std::cout << "Restricted to genres:";
        for (const std::string& name : genres) std::cout << " " << name;
        std::cout << std::endl;
        if (!recommender.setGenreIds(catalogue.genreIds)) return false;
    }
    const std::vector<int> recs = recommender.recommendScaled(members, topN, scales, euclidean, ranges, genreIds);
    if (recs.empty()) {
        std::cerr << "No recommendations found. Please check the query." << std::endl;
        return false;
    }
    const std::vector<float> distances = recommender.lastScores();
    std::map<int, std::string>& genreMap = catalogue.genreMap;
    Song song;
    std::cout << "\n----------------------------------------------\n" << (isPlaylist ? "Playlist" : "Query") << " (" << members.size()
              << (members.size() == 1 ? " song):" : " songs):") << std::endl;
    for (size_t i = 0; i < members.size(); ++i) {
        if (!DataManager::readSong(catalogue, static_cast<size_t>(members[i]), song)) {
            std::cerr << "Error: could not read song " << members[i] << " from " << catalogue.path << std::endl;
            return false;
        }
        std::cout << "  " << (i + 1) << ". \"" << song.track_name << "\"" << std::endl;
        printSong(song, genreMap, "     ");
    }
    std::cout << "----------------------------------------------" << std::endl;
    std::cout << "\nTop " << recs.size() << " Recommendations:\n" << std::endl;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (!DataManager::readSong(catalogue, static_cast<size_t>(recs[i]), song)) {
            std::cerr << "Error: could not read song " << recs[i] << " from " << catalogue.path << std::endl;
            return false;
        }
        std::cout << (i + 1) << ". \"" << song.track_name << "\"  (" << (euclidean ? "distance " : "score ") << distances[i] << ")" << std::endl;
        printSong(song, genreMap, "   ");
        if (i + 1 < recs.size()) std::cout << std::endl;
    }
    std::cout << "\nRecommendation complete!" << std::endl;
    return true;
}

int main(int argc, char* argv[]) {
    std::cout << "== High-Performance Music Recommendation Engine ==\n"
              << "==   MI355X-native (HIP / gfx950) cosine top-N  ==\n" << std::endl;
    if (argc < 2) {
        usage(argv[0]);
        return 1;
    }
    const std::string mode = argv[1];
    if (mode == "--preprocess") {
        if (argc < 3) {
            std::cerr << "Error: CSV path required for preprocessing mode" << std::endl;
            usage(argv[0]);
            return 1;
        }
        return preprocessMode(argv[2]) ? 0 : 1;
    }
    if (mode == "--song" || mode == "--id") {
        if (argc < 3) {
            std::cerr << "Error: Song name or track ID required" << std::endl;
            usage(argv[0]);
            return 1;
        }
        int topN = 10;
        for (int i = 3; i < argc - 1; ++i) {  // main.cpp:169-178
            if (std::strcmp(argv[i], "-n") == 0) {
                topN = std::atoi(argv[i + 1]);
                if (topN <= 0) {
                    std::cerr << "Error: Invalid value for -n (must be positive)" << std::endl;
                    return 1;
                }
                break;
            }
        }
        std::vector<std::string> genres;   // --genre NAME, any number of times
        for (int i = 3; i < argc; ++i) {
            if (std::strcmp(argv[i], "--genre") != 0) continue;
            if (i + 1 >= argc) {
                std::cerr << "Error: --genre needs a genre name" << std::endl;
                return 1;
            }
            genres.push_back(argv[++i]);
        }
        std::vector<Recommender::FeatureRange> ranges;
        if (!parseWhere(argc, argv, 3, ranges)) return 1;
        if (!parseRowSet(argc, argv, 3, g_rowSet)) return 1;
        bool euclidean = false;
        if (!parseMetric(argc, argv, 3, euclidean)) return 1;
        std::vector<float> scales;
        if (!parseScale(argc, argv, 3, scales)) return 1;
        if (euclidean || !scales.empty()) return nearestMode(argv[2], false, mode == "--id", topN, ranges, genres, euclidean, scales) ? 0 : 1;
        if (!ranges.empty() && !genres.empty()) {
            std::cerr << "Error: --where cannot be combined with --genre" << std::endl;
            return 1;
        }
        if (g_rowSet.on && !genres.empty()) {
            std::cerr << "Error: " << (g_rowSet.only ? "--only" : "--seen") << " cannot be combined with --genre here: use --playlist <one id> --genre ..."
                      << std::endl;
            return 1;
        }
        DiverseOpt dv;
        if (!parseDiverse(argc, argv, 3, topN, dv)) return 1;
        if (dv.on && !genres.empty()) {
            std::cerr << "Error: " << (dv.maxPerArtist > 0 ? "--max-per-artist" : "--diverse") << " cannot be combined with --genre" << std::endl;
            return 1;
        }
        return recommendationMode(argv[2], mode == "--id", topN, genres, ranges, dv) ? 0 : 1;
    }
    if (mode == "--playlist") {
        if (argc < 3) {
            std::cerr << "Error: --playlist needs a comma-separated list of track IDs" << std::endl;
            return 1;
        }
        int topN = 10;
        for (int i = 3; i < argc - 1; ++i) {
            if (std::strcmp(argv[i], "-n") == 0) {
                topN = std::atoi(argv[i + 1]);
                if (topN <= 0) {
                    std::cerr << "Error: Invalid value for -n (must be positive)" << std::endl;
                    return 1;
                }
                break;
            }
        }
        std::vector<Recommender::FeatureRange> ranges;
        if (!parseWhere(argc, argv, 3, ranges)) return 1;
        if (!parseRowSet(argc, argv, 3, g_rowSet)) return 1;
        bool euclidean = false;
        if (!parseMetric(argc, argv, 3, euclidean)) return 1;
        std::vector<float> scales;
        if (!parseScale(argc, argv, 3, scales)) return 1;
        if (euclidean || !scales.empty()) {
            std::vector<std::string> in_genres;
            for (int i = 3; i < argc; ++i) {
                if (std::strcmp(argv[i], "--genre") != 0) continue;
                if (i + 1 >= argc) {
                    std::cerr << "Error: --genre needs a genre name" << std::endl;
                    return 1;
                }
                in_genres.push_back(argv[++i]);
            }
            return nearestMode(argv[2], true, true, topN, ranges, in_genres, euclidean, scales) ? 0 : 1;
        }
        Taste taste;
        if (!parseTaste(argc, argv, 3, taste)) return 1;
        DiverseOpt dv;
        if (!parseDiverse(argc, argv, 3, topN, dv)) return 1;
        std::vector<std::string> genres;   // --genre NAME, any number of times
        for (int i = 3; i < argc; ++i) {
            if (std::strcmp(argv[i], "--genre") != 0) continue;
            if (i + 1 >= argc) {
                std::cerr << "Error: --genre needs a genre name" << std::endl;
                return 1;
            }
            genres.push_back(argv[++i]);
        }
        PriorOpt pr;
        if (!parsePrior(argc, argv, 3, pr)) return 1;
        return playlistMode(argv[2], topN, ranges, taste, dv, genres, pr) ? 0 : 1;
    }
    std::cerr << "Error: Unknown mode '" << mode << "'" << std::endl;
    usage(argv[0]);
    return 1;
}
