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
//   ... --song, --id and --playlist with --distance manhattan: the NEAREST songs by Manhattan (L1) distance over the 12 features,
//       for a playlist the mean of the distances to its songs (extension; with --genre, --where, --seen and --only and nothing else;
//       distances are printed; --metric keeps its two names)
//   ... --song, --id and --playlist with --min-score S: only the songs whose similarity is at least S, and "N of TOTAL matching":
//       how many songs of the catalogue pass, whatever -n is; with --metric euclidean it is --within R: the songs within distance R
//       (extension: BOUNDED REQUESTS; with --genre, --where, --seen and --only and nothing else; --count-only prints the number alone)
//   ... --song, --id and --playlist with --similarity jaccard: the MOST SIMILAR songs by weighted (Ruzicka) Jaccard similarity over the
//       12 features, sum min / sum max, for a playlist the mean of the similarities to its songs (extension; with --genre, --where,
//       --seen and --only and nothing else; similarities are printed; --metric and --distance keep their names)
//   ... --song, --id and --playlist with one or more --scale NAME=S: feature NAME counts S times (0: ignored) in the similarity or
//       the distance (extension; under both metrics, with --genre and --where)
//   ... the same modes with --candidates FILE (track ids, one per line, as for --only): only the listed songs are READ and ranked (a
//       candidate list: the engine gathers them and makes no pass over the catalogue); goes with --seen or --only; extension
//   ... the same modes with --score FILE (track ids, one per line, as for --candidates): nothing is recommended; every listed track
//       is printed in file order with the request's value for it (its score, or its distance under --metric euclidean), or "not
//       eligible" where the request can never return it (a song of the query, a --seen song, outside --where or --genre); -n is
//       ignored; "how similar is song A to song B" is --id A --score <file naming B>; goes with --seen, --only, --where, --scale,
//       --metric and the --playlist mode's weights, genres and priors; not with --candidates, --diverse, --max-per-artist or --pool,
//       nor with --genre under --song / --id; extension
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
#include <sstream>
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

static const char* const kScaleNames[] = {"danceability", "energy", "key", "loudness", "mode", "speechiness",
                                          "acousticness", "instrumentalness", "liveness", "valence", "tempo", "genre"};

// --scale NAME=S, any number of times from argv[first]: scales = 12 factors in Song.h order (1 where not named), or empty when the
// option is not given.  false, with a message, on a malformed option or an unknown NAME.
static bool parseScale(int argc, char* argv[], int first, std::vector<float>& scales) {
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
            if (name == kScaleNames[j]) feature = j;
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
    return true;
}

// The scales that are not 1, announced (none given: nothing).
static void printScales(const std::vector<float>& scales) {
    if (scales.empty()) return;
    std::cout << "Feature scales:";
    for (int j = 0; j < 12; ++j)
        if (scales[static_cast<size_t>(j)] != 1.0f) std::cout << " " << kScaleNames[j] << "=" << scales[static_cast<size_t>(j)];
    std::cout << std::endl;
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

// --seen FILE / --only FILE from argv[first] (row sets).
struct RowSetOpt {
    bool on = false, only = false;
    std::string file;
};

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

// --candidates FILE from argv[first] (candidate lists): the format of --only FILE; goes with --seen or --only.
struct CandidatesOpt {
    bool on = false;
    std::string file;
};

static bool parseCandidates(int argc, char* argv[], int first, CandidatesOpt& c) {
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--candidates") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --candidates needs a file of track ids (one per line)" << std::endl;
            return false;
        }
        if (c.on) {
            std::cerr << "Error: --candidates is given once (a request takes one candidate list)" << std::endl;
            return false;
        }
        c.on = true;
        c.file = argv[++i];
    }
    return true;
}

// --score FILE from argv[first] (candidate scores): the format of --candidates FILE.  The listed tracks are not ranked: each is
// printed with the request's value for it.  Not with --candidates (the file IS the list), nor with a re-rank (--diverse,
// --max-per-artist, --pool: a re-ranked order has no value per track).
struct ScoreOpt {
    bool on = false;
    std::string file;
};

static bool parseScore(int argc, char* argv[], int first, ScoreOpt& sc) {
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--score") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --score needs a file of track ids (one per line)" << std::endl;
            return false;
        }
        if (sc.on) {
            std::cerr << "Error: --score is given once (a request scores one list)" << std::endl;
            return false;
        }
        sc.on = true;
        sc.file = argv[++i];
    }
    if (!sc.on) return true;
    for (int i = first; i < argc; ++i)
        for (const char* other : {"--candidates", "--diverse", "--max-per-artist", "--pool"})
            if (std::strcmp(argv[i], other) == 0) {
                std::cerr << "Error: --score cannot be combined with " << other
                          << (std::strcmp(other, "--candidates") == 0 ? " (the scored file is the list)" : " (a re-ranked order has no value per track)")
                          << std::endl;
                return false;
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

// The rows of the track ids in `file` (one per line, blank lines skipped, the first row of an id as for --id) appended to `rows`; a line
// that names no song of the catalogue is counted in `skipped`.  false, with a message that calls the file `what`, when it cannot be opened.
static bool readTrackIdFile(const DataManager::Catalogue& catalogue, const std::string& file, const char* what, std::vector<int>& rows,
                            size_t& skipped) {
    std::ifstream in(file);
    if (!in) {
        std::cerr << "Error: cannot open the " << what << " file '" << file << "'" << std::endl;
        return false;
    }
    std::unordered_map<std::string, int> byId;
    for (size_t i = 0; i < catalogue.size(); ++i) byId.emplace(catalogue.trackIds[i], static_cast<int>(i));   // (the first row of an id)
    skipped = 0;
    std::string line;
    while (std::getline(in, line)) {
        const size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        const auto hit = byId.find(line.substr(a, line.find_last_not_of(" \t\r") - a + 1));
        if (hit == byId.end()) ++skipped;
        else rows.push_back(hit->second);
    }
    return true;
}

// --seen / --only: the file's track ids (one per line, blank lines skipped, the first row of an id as for --id) to the recommender
// as its row set.  A line that names no song of the catalogue is skipped; how many were is said on stderr (a history normally
// holds tracks the catalogue lacks).  false, with a message, when the file cannot be read or the set is refused.
static bool applyRowSet(Recommender& recommender, const DataManager::Catalogue& catalogue, const RowSetOpt& rs) {
    if (!rs.on) return true;
    std::vector<int> rows;
    size_t skipped = 0;
    if (!readTrackIdFile(catalogue, rs.file, "row set", rows, skipped)) return false;
    std::cerr << "Row set (" << (rs.only ? "--only" : "--seen") << " " << rs.file << "): " << rows.size() << " tracks, " << skipped
              << " lines skipped (not in the catalogue)" << std::endl;
    if (!recommender.setRowSet(rows, rs.only)) return false;
    std::cout << (rs.only ? "Only among " : "Leaving out ") << rows.size() << " listed songs" << std::endl;
    return true;
}

// --candidates: the file's track ids (the rules of --only FILE) to the recommender as its candidate list: only they are read and
// ranked.  false, with a message, when the file cannot be read or the list is refused.
static bool applyCandidates(Recommender& recommender, const DataManager::Catalogue& catalogue, const CandidatesOpt& c) {
    if (!c.on) return true;
    std::vector<int> rows;
    size_t skipped = 0;
    if (!readTrackIdFile(catalogue, c.file, "candidate list", rows, skipped)) return false;
    std::cerr << "Candidate list (--candidates " << c.file << "): " << rows.size() << " tracks, " << skipped
              << " lines skipped (not in the catalogue)" << std::endl;
    if (!recommender.setCandidates(std::vector<int64_t>(rows.begin(), rows.end()))) return false;
    std::cout << "Ranking " << rows.size() << " listed candidates" << std::endl;
    return true;
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

// --metric NAME from argv[first]: euclidean = true for "euclidean", false for "cosine" or no option.  false (the return
// value), with a message, for another name.
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
    return true;
}

// --match NAME from argv[first]: anyOf = true for "any" (ANY-OF REQUESTS: rank by the best-matching playlist song), false for "mean"
// or no option.  false (the return value), with a message, for another name or without --playlist.
static bool parseMatch(int argc, char* argv[], int first, bool playlist, bool& anyOf) {
    anyOf = false;
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--match") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --match needs a name (mean or any)" << std::endl;
            return false;
        }
        const std::string name = argv[++i];
        if (name != "mean" && name != "any") {
            std::cerr << "Error: --match '" << name << "': mean or any" << std::endl;
            return false;
        }
        if (!playlist) {
            std::cerr << "Error: --match goes with --playlist" << std::endl;
            return false;
        }
        anyOf = name == "any";
    }
    return true;
}

// --distance NAME from argv[first]: manhattan = true for "manhattan" (MANHATTAN REQUESTS: the nearest songs by L1 distance), false
// without the option.  false (the return value), with a message, for another name.
static bool parseDistance(int argc, char* argv[], int first, bool& manhattan) {
    manhattan = false;
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--distance") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --distance needs a name (manhattan)" << std::endl;
            return false;
        }
        const std::string name = argv[++i];
        if (name != "manhattan") {
            std::cerr << "Error: --distance '" << name << "': manhattan" << std::endl;
            return false;
        }
        manhattan = true;
    }
    return true;
}

// --similarity NAME from argv[first]: jaccard = true for "jaccard" (JACCARD REQUESTS: the most similar songs by weighted Jaccard
// similarity), false without the option.  false (the return value), with a message, for another name.
static bool parseSimilarity(int argc, char* argv[], int first, bool& jaccard) {
    jaccard = false;
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--similarity") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --similarity needs a name (jaccard)" << std::endl;
            return false;
        }
        const std::string name = argv[++i];
        if (name != "jaccard") {
            std::cerr << "Error: --similarity '" << name << "': jaccard" << std::endl;
            return false;
        }
        jaccard = true;
    }
    return true;
}

// --min-score S, --within R and --count-only from argv[first] (BOUNDED REQUESTS): bounded = true with `bound` = S or R.  false (the
// return value), with a message, for a value that is no finite number, both options, --within without --metric euclidean,
// --min-score with it, or --count-only without either.
static bool parseBound(int argc, char* argv[], int first, bool euclidean, bool& bounded, float& bound, bool& countOnly) {
    bounded = countOnly = false;
    const char* which = nullptr;
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--count-only") == 0) countOnly = true;
        if (std::strcmp(argv[i], "--min-score") != 0 && std::strcmp(argv[i], "--within") != 0) continue;
        const char* option = argv[i];
        if (i + 1 >= argc) {
            std::cerr << "Error: " << option << " needs a number" << std::endl;
            return false;
        }
        if (which) {
            std::cerr << "Error: " << option << " cannot be combined with " << which << " (one bound per request)" << std::endl;
            return false;
        }
        char* end = nullptr;
        const float v = std::strtof(argv[++i], &end);
        if (end == argv[i] || *end != '\0' || !(v - v == 0.0f)) {
            std::cerr << "Error: " << option << " '" << argv[i] << "': a finite number" << std::endl;
            return false;
        }
        which = option;
        bounded = true;
        bound = v;
    }
    if (which && (std::strcmp(which, "--within") == 0) != euclidean) {
        std::cerr << "Error: " << (euclidean ? "--min-score cannot be combined with --metric euclidean (a radius is --within R)"
                                             : "--within goes with --metric euclidean (a score floor is --min-score S)")
                  << std::endl;
        return false;
    }
    if (bounded && euclidean && bound < 0.0f) {
        std::cerr << "Error: --within '" << bound << "': a radius is >= 0" << std::endl;
        return false;
    }
    if (countOnly && !bounded) {
        std::cerr << "Error: --count-only goes with --min-score or --within" << std::endl;
        return false;
    }
    return true;
}

// -n N: the first -n among argv[first .. argc-2] (the reference's rule, main.cpp:169-178: in last position it is not looked at).
static bool parseTopN(int argc, char* argv[], int first, int& topN) {
    for (int i = first; i < argc - 1; ++i) {
        if (std::strcmp(argv[i], "-n") != 0) continue;
        topN = std::atoi(argv[i + 1]);
        if (topN <= 0) {
            std::cerr << "Error: Invalid value for -n (must be positive)" << std::endl;
            return false;
        }
        break;
    }
    return true;
}

// --genre NAME, any number of times from argv[first].
static bool parseGenres(int argc, char* argv[], int first, std::vector<std::string>& genres) {
    for (int i = first; i < argc; ++i) {
        if (std::strcmp(argv[i], "--genre") != 0) continue;
        if (i + 1 >= argc) {
            std::cerr << "Error: --genre needs a genre name" << std::endl;
            return false;
        }
        genres.push_back(argv[++i]);
    }
    return true;
}

// Everything a query mode's command line says.
struct Options {
    bool playlist = false;     // --playlist (else --song / --id)
    bool isTrackId = false;    // the query names track ids (--id, --playlist), not a song name
    std::string query;
    int topN = 10;
    std::vector<std::string> genres;
    std::vector<Recommender::FeatureRange> ranges;
    RowSetOpt rowSet;
    CandidatesOpt candidates;
    ScoreOpt score;
    bool euclidean = false;
    bool anyOf = false;        // --match any
    bool manhattan = false;    // --distance manhattan
    bool jaccard = false;      // --similarity jaccard
    bool bounded = false;      // --min-score S, or --within R under --metric euclidean: `bound`
    float bound = 0.0f;
    bool countOnly = false;    // --count-only
    std::vector<float> scales;
    Taste taste;
    DiverseOpt dv;
    PriorOpt pr;
    // a distance or scaled request (its own banner; scores or distances are printed; --song / --id run as the one-song playlist)
    bool nearest() const { return euclidean || manhattan || jaccard || bounded || !scales.empty(); }
};

// What does not combine: the option `given` stands for beside one of `beside` (the first of them in argv stands for %s in `text`).
// A row is looked at where its `given` has just been parsed (parseOptions), so that a command line with two faults reports the
// one it always reported.  (--seen beside --only, or either twice, is refused where they are parsed: parseRowSet; --pool without
// --diverse or a cap in parseDiverse.)
enum class Given {
    Euclidean,       // --metric euclidean
    Scale,           // --scale
    GenreFiltered,   // --genre under --song / --id by unscaled cosine, beside a filter or a row set ...
    GenreReranked,   // ... and beside a re-rank: --playlist <one id> and the distance and scaled requests serve those pairs
    MatchAny,        // --match any
    Manhattan,       // --distance manhattan
    Bounded,         // --min-score, --within
    Jaccard,         // --similarity jaccard
};
struct Refusal {
    Given given;
    std::vector<const char*> beside;
    const char* text;
};
static const std::vector<const char*> kRequestOptions = {"--diverse",        "--pool",   "--weights",      "--dislike",
                                                         "--dislike-weight", "--priors", "--prior-weight", "--max-per-artist"};
static const Refusal kRefusals[] = {
    {Given::Euclidean, kRequestOptions, "--metric euclidean cannot be combined with %s (distance requests take --genre and --where only)"},
    {Given::Scale, kRequestOptions, "--scale cannot be combined with %s (scaled requests take --metric, --genre and --where only)"},
    {Given::GenreFiltered, {"--where"}, "%s cannot be combined with --genre"},
    {Given::GenreFiltered, {"--seen", "--only", "--candidates", "--score"}, "%s cannot be combined with --genre here: use --playlist <one id> --genre ..."},
    {Given::GenreReranked, {"--max-per-artist"}, "%s cannot be combined with --genre"},
    {Given::GenreReranked, {"--diverse"}, "%s cannot be combined with --genre"},
    {Given::MatchAny, kRequestOptions, "--match any cannot be combined with %s (any-of requests take --genre, --where, --seen and --only only)"},
    {Given::MatchAny, {"--scale", "--candidates", "--score"}, "--match any cannot be combined with %s (any-of requests take --genre, --where, --seen and --only only)"},
    {Given::Manhattan, kRequestOptions, "--distance manhattan cannot be combined with %s (Manhattan requests take --genre, --where, --seen and --only only)"},
    {Given::Manhattan, {"--scale", "--candidates", "--score"}, "--distance manhattan cannot be combined with %s (Manhattan requests take --genre, --where, --seen and --only only)"},
    {Given::Bounded, kRequestOptions, "a bound (--min-score, --within) cannot be combined with %s (bounded requests take --genre, --where, --seen and --only only)"},
    {Given::Bounded, {"--scale", "--candidates", "--score"},"a bound (--min-score, --within) cannot be combined with %s (bounded requests take --genre, --where, --seen and --only only)"},
    {Given::Jaccard, kRequestOptions, "--similarity jaccard cannot be combined with %s (Jaccard requests take --genre, --where, --seen and --only only)"},
    {Given::Jaccard, {"--scale", "--candidates", "--score", "--metric", "--distance", "--match", "--min-score", "--within", "--count-only"}, "--similarity jaccard cannot be combined with %s (Jaccard requests take --genre, --where, --seen and --only only)"},
};

// true, with the message, when `given` holds and the command line has an option that one of its rows refuses beside it.
static bool refused(int argc, char* argv[], int first, const Options& o, Given given) {
    const bool genreAlone = !o.playlist && !o.nearest() && !o.genres.empty();
    if (!(given == Given::Euclidean ? o.euclidean : given == Given::Scale ? !o.scales.empty() : given == Given::MatchAny ? o.anyOf : given == Given::Manhattan ? o.manhattan : given == Given::Bounded ? o.bounded : given == Given::Jaccard ? o.jaccard : genreAlone))
        return false;
    for (const Refusal& r : kRefusals) {
        if (r.given != given) continue;
        for (int i = first; i < argc; ++i)
            for (const char* other : r.beside)
                if (std::strcmp(argv[i], other) == 0) {
                    std::string text = r.text;
                    std::cerr << "Error: " << text.replace(text.find("%s"), 2, other) << std::endl;
                    return true;
                }
    }
    return false;
}

// The options of a query mode from argv[3..], each by its own parser, in the order that decides which malformed option is
// reported first (--song / --id look at --genre first, --playlist after its other options).  false: the message is out.
static bool parseOptions(int argc, char* argv[], Options& o) {
    const int first = 3;
    o.playlist = std::strcmp(argv[1], "--playlist") == 0;
    o.isTrackId = std::strcmp(argv[1], "--song") != 0;
    o.query = argv[2];
    if (!parseTopN(argc, argv, first, o.topN)) return false;
    if (!o.playlist && !parseGenres(argc, argv, first, o.genres)) return false;
    if (!parseWhere(argc, argv, first, o.ranges) || !parseRowSet(argc, argv, first, o.rowSet)) return false;
    if (!parseCandidates(argc, argv, first, o.candidates) || !parseScore(argc, argv, first, o.score)) return false;
    if (!parseSimilarity(argc, argv, first, o.jaccard) || refused(argc, argv, first, o, Given::Jaccard)) return false;
    if (!parseMetric(argc, argv, first, o.euclidean) || refused(argc, argv, first, o, Given::Euclidean)) return false;
    if (!parseMatch(argc, argv, first, o.playlist, o.anyOf) || refused(argc, argv, first, o, Given::MatchAny)) return false;
    if (o.anyOf && o.euclidean) {
        std::cerr << "Error: --match any cannot be combined with --metric euclidean (any-of requests take --genre, --where, --seen and --only only)"
                  << std::endl;
        return false;
    }
    if (!parseDistance(argc, argv, first, o.manhattan) || refused(argc, argv, first, o, Given::Manhattan)) return false;
    if (o.manhattan && (o.euclidean || o.anyOf)) {
        std::cerr << "Error: --distance manhattan cannot be combined with " << (o.euclidean ? "--metric euclidean" : "--match any")
                  << " (Manhattan requests take --genre, --where, --seen and --only only)" << std::endl;
        return false;
    }
    if (!parseBound(argc, argv, first, o.euclidean, o.bounded, o.bound, o.countOnly) || refused(argc, argv, first, o, Given::Bounded)) return false;
    if (o.bounded && (o.anyOf || o.manhattan)) {
        std::cerr << "Error: a bound (--min-score, --within) cannot be combined with " << (o.anyOf ? "--match any" : "--distance manhattan")
                  << " (bounded requests take --genre, --where, --seen and --only only)" << std::endl;
        return false;
    }
    if (!parseScale(argc, argv, first, o.scales) || refused(argc, argv, first, o, Given::Scale)) return false;
    printScales(o.scales);
    if (refused(argc, argv, first, o, Given::GenreFiltered)) return false;
    if (o.playlist && !parseTaste(argc, argv, first, o.taste)) return false;
    if (!parseDiverse(argc, argv, first, o.topN, o.dv) || refused(argc, argv, first, o, Given::GenreReranked)) return false;
    return !o.playlist || (parseGenres(argc, argv, first, o.genres) && parsePrior(argc, argv, first, o.pr));
}

// One recommended (or member) song's lines.
static bool printEntry(const DataManager::Catalogue& catalogue, std::map<int, std::string>& genreMap, int row, size_t number,
                       const char* indent, const std::string& suffix) {
    Song song;
    if (!DataManager::readSong(catalogue, static_cast<size_t>(row), song)) {
        std::cerr << "Error: could not read song " << row << " from " << catalogue.path << std::endl;
        return false;
    }
    std::cout << indent << number << ". \"" << song.track_name << "\"" << suffix << std::endl;
    printSong(song, genreMap, *indent ? "     " : "   ");
    return true;
}

// The rows of the songs named (track ids, or a song name by the engine's rules); false, with a message, for one that is not there.
static bool resolveMembers(const DataManager::Catalogue& catalogue, const std::vector<std::string>& names, bool isTrackId,
                           std::vector<int>& members) {
    for (const std::string& name : names) {
        const int index = findQuery(catalogue, name, isTrackId);
        if (index < 0) {
            std::cerr << "Error: Song with " << (isTrackId ? "track_id" : "name") << " '" << name << "' not found" << std::endl;
            return false;
        }
        members.push_back(index);
    }
    return true;
}

// Artist groups, genre ids and priors to the recommender, each announced.  oneLine: --song / --id say cap and lambda on one line.
static bool handOver(Recommender& recommender, const DataManager::Catalogue& catalogue, const Options& o, bool oneLine,
                     const std::vector<int>& genreIds) {
    const DiverseOpt& dv = o.dv;
    if (dv.maxPerArtist > 0) {
        if (!capByArtist(recommender, catalogue)) return false;
        std::cout << "At most " << dv.maxPerArtist << " per artist";
        if (oneLine && dv.lambda < 1.0f) std::cout << "; diversified: lambda " << dv.lambda;
        std::cout << std::endl;
    }
    if (dv.on && (dv.maxPerArtist == 0 || (!oneLine && dv.lambda < 1.0f))) std::cout << "Diversified: lambda " << dv.lambda << std::endl;
    if (!genreIds.empty()) {
        std::cout << "Restricted to genres:";
        for (const std::string& name : o.genres) std::cout << " " << name;
        std::cout << std::endl;
        if (!recommender.setGenreIds(catalogue.genreIds)) return false;
    }
    if (o.pr.on) {
        std::vector<float> priors;
        if (!readPriors(o.pr.file, catalogue.size(), priors) || !recommender.setPriors(priors)) return false;
        std::cout << "Prior weight: " << o.pr.weight << " (" << o.pr.file << ")" << std::endl;
    }
    return true;
}

// The "Query Song" block of --song / --id.  The reference finds the song it DISPLAYS with a single exact-or-substring
// pass (main.cpp:85-95), not the engine's exact-then-substring rule; kept.
static void printQuerySong(const DataManager::Catalogue& catalogue, std::map<int, std::string>& genreMap, const Options& o) {
    int shown = -1;
    const std::string needle = lowered(o.query);
    for (size_t i = 0; i < catalogue.size() && shown < 0; ++i) {
        const std::string name = o.isTrackId ? std::string() : lowered(catalogue.trackNames[i]);
        if (o.isTrackId ? catalogue.trackIds[i] == o.query : name == needle || name.find(needle) != std::string::npos) shown = static_cast<int>(i);
    }
    Song s;
    if (shown < 0 || !DataManager::readSong(catalogue, static_cast<size_t>(shown), s)) return;
    std::cout << "\n----------------------------------------------\nQuery Song:\n"
              << "  Title:   " << s.track_name << "\n"
              << "  Artist:  " << s.artists << "\n"
              << "  Genre:   " << genreMap[s.genre_id] << "\n"
              << "  ID:      " << s.track_id
              << "\n----------------------------------------------" << std::endl;
}

// The query modes (main.cpp:46-131 and the extensions): load the catalogue, resolve the member songs, initialise, apply the row
// set, hand over genre ids, artist groups and priors, ask, print.  Three flavours differ in what they print and in when they
// look their songs up: --song / --id by unscaled cosine ("song": the reference's mode; the song is looked up after initialize
// and whatever goes wrong from there ends in "No recommendations found"), --playlist, and the distance or scaled request of any.
static bool queryMode(const Options& o) {
    const bool nearest = o.nearest(), song = !o.playlist && !nearest;
    std::cout << (nearest ? (o.bounded     ? (o.euclidean ? "=== BOUNDED MODE (within a Euclidean distance) ===" : "=== BOUNDED MODE (similarity at least a score) ===")
                             : o.jaccard   ? "=== RECOMMENDATION MODE (Jaccard similarity) ==="
                             : o.manhattan ? "=== NEAREST MODE (Manhattan distance) ==="
                             : o.euclidean ? "=== NEAREST MODE (Euclidean distance) ==="
                                           : "=== SCALED MODE (cosine over scaled features) ===")
                  : song  ? "=== RECOMMENDATION MODE ==="
                          : "=== PLAYLIST MODE ===")
              << std::endl;
    const auto noRecommendations = [] {
        std::cerr << "No recommendations found. Please check the query." << std::endl;
        return false;
    };
    const auto namesNoTrack = [] {
        std::cerr << "Error: the playlist names no track" << std::endl;
        return false;
    };

    // 1. the catalogue (--playlist looks at its list before it opens it, a distance or scaled request after)
    std::vector<std::string> names = o.playlist ? splitList(o.query) : std::vector<std::string>{o.query};
    if (names.empty() && !nearest) return namesNoTrack();
    DataManager::Catalogue catalogue;
    if (!DataManager::loadCatalogue(kBinaryDataFile, catalogue)) {
        std::cerr << "Failed to load data. Have you run preprocessing?" << std::endl;
        return false;
    }
    std::map<int, std::string>& genreMap = catalogue.genreMap;

    // 2. the member songs and their weights (the disliked songs are members with a negative weight)
    const Taste& taste = o.taste;
    if (taste.haveWeights && taste.weights.size() != names.size()) {
        std::cerr << "Error: --weights names " << taste.weights.size() << " weights for " << names.size() << " playlist songs" << std::endl;
        return false;
    }
    std::vector<int> genreIds, members;   // --genre: only songs of these genres are recommended (the members may be of any)
    if (!song && !genreIdsOf(catalogue, o.genres, genreIds)) return false;
    if (names.empty()) return namesNoTrack();
    std::vector<float> weights = taste.haveWeights ? taste.weights : std::vector<float>(names.size(), 1.0f);
    weights.insert(weights.end(), taste.dislike.size(), -taste.dislikeWeight);
    names.insert(names.end(), taste.dislike.begin(), taste.dislike.end());
    if (!song && !resolveMembers(catalogue, names, o.isTrackId, members)) return false;

    // 3. the engine, 4. the row set
    Recommender recommender;
    if (!recommender.initialize(catalogue.features, catalogue.trackIds, catalogue.trackNames)) {
        std::cerr << "Failed to initialize recommender" << std::endl;
        return false;
    }
    if (!applyRowSet(recommender, catalogue, o.rowSet) || !applyCandidates(recommender, catalogue, o.candidates)) return false;

    // (2. for the song flavour.)  Without an extension option it is the reference's own route: recommend / recommendByName look
    // the song up themselves; with --genre alone its label-scan form.  Everything else is one Recommender::Query.
    const bool reference = song && !o.dv.on && o.ranges.empty() && !o.rowSet.on && !o.candidates.on && !o.score.on;
    if (song) {
        std::cout << "\nSearching for " << (o.isTrackId ? "track ID: " : "song: ") << o.query << std::endl;
        if (!genreIdsOf(catalogue, o.genres, genreIds)) return false;
        if ((!reference || !genreIds.empty()) && !resolveMembers(catalogue, names, o.isTrackId, members)) return noRecommendations();
    }

    // 5. genre ids, artist groups, priors
    if (!handOver(recommender, catalogue, o, song, genreIds)) return song ? noRecommendations() : false;

    // 6. the request
    std::vector<int> recs;
    std::vector<int64_t> listed;   // --score: the file's tracks, and the request's value of each
    std::vector<float> listedValues;
    std::vector<char> eligible;
    if (o.score.on) {
        std::vector<int> rows;
        size_t skipped = 0;
        if (!readTrackIdFile(catalogue, o.score.file, "score list", rows, skipped)) return false;
        std::cerr << "Score list (--score " << o.score.file << "): " << rows.size() << " tracks, " << skipped
                  << " lines skipped (not in the catalogue)" << std::endl;
        listed.assign(rows.begin(), rows.end());
        std::cout << "Scoring " << listed.size() << " listed tracks" << std::endl;
    }
    if (reference && genreIds.empty()) {
        recs = o.isTrackId ? recommender.recommend(o.query, o.topN) : recommender.recommendByName(o.query, o.topN);
    } else if (reference) {
        recs = recommender.recommendByIndexInGenres(members[0], o.topN, genreIds);
    } else {
        Recommender::Query q;
        q.songs = members;
        // (--song / --id keep recommendByIndex's clamp: the reference's heap never holds more than N-1 entries)
        q.topN = song ? std::min(o.topN, static_cast<int>(catalogue.size()) - 1) : o.topN;
        if (taste.weighted) q.weights = weights;
        q.where = o.ranges;
        q.genreIds = genreIds;
        q.diverse = o.dv.on;
        q.lambda = o.dv.lambda;
        q.pool = o.dv.pool;
        q.maxPerArtist = o.dv.maxPerArtist;
        q.priorWeight = o.pr.on ? o.pr.weight : 0.0f;   // (BETA 0 is the call without a prior)
        q.scales = o.scales;
        q.euclidean = o.euclidean;
        q.anyOf = o.anyOf;
        q.manhattan = o.manhattan;
        q.jaccard = o.jaccard;
        if (o.bounded) {   // BOUNDED REQUESTS: the leading matches and the number of matching songs; --count-only asks for no song
            if (o.euclidean) q.within(o.bound);
            else q.atLeast(o.bound);
            if (o.countOnly) q.topN = 0;
        }
        if (o.score.on) listedValues = recommender.scoreSongs(q, listed, &eligible);
        else if (q.topN > 0 || o.bounded) recs = recommender.recommendQuery(q);
    }
    const long long matching = o.bounded ? recommender.lastMatchCount() : -1;   // (a bounded request may match nothing: that is an answer)
    if (o.score.on ? listedValues.size() != listed.size() || listed.empty() : recs.empty() && matching < 0) return noRecommendations();

    // 7. the query's block, then the recommendations (a distance or scaled request prints their values)
    const std::vector<float> values = recommender.lastScores();
    const std::vector<int> matched = recommender.lastMatchedSongs();   // --match any: the playlist song each recommendation matched
    if (song) {
        printQuerySong(catalogue, genreMap, o);
    } else {
        std::cout << "\n----------------------------------------------\n" << (o.playlist ? "Playlist" : "Query") << " (" << members.size()
                  << (nearest && members.size() == 1 ? " song):" : " songs):") << std::endl;
        for (size_t i = 0; i < members.size(); ++i) {
            std::ostringstream weight;
            if (taste.weighted) weight << "  (weight " << weights[i] << ")";
            if (!printEntry(catalogue, genreMap, members[i], i + 1, "  ", weight.str())) return false;
        }
        std::cout << "----------------------------------------------" << std::endl;
        if (o.anyOf) std::cout << "Matching: the best of the playlist's songs (--match any)" << std::endl;
    }
    if (o.score.on) {   // --score: the listed tracks in file order, nothing is recommended
        std::cout << "\nValues of " << listed.size() << " listed tracks:\n" << std::endl;
        for (size_t i = 0; i < listed.size(); ++i) {
            std::ostringstream value;
            if (eligible[i]) value << "  (" << (o.euclidean ? "distance " : "score ") << listedValues[i] << ")";
            else value << "  (not eligible)";
            if (!printEntry(catalogue, genreMap, static_cast<int>(listed[i]), i + 1, "", value.str())) return false;
            if (i + 1 < listed.size()) std::cout << std::endl;
        }
        std::cout << "\nScoring complete!" << std::endl;
        return true;
    }
    if (o.bounded) {
        std::cout << "\n" << recs.size() << " of " << matching << " matching (" << (o.euclidean ? "distance <= " : "score >= ") << o.bound << ")"
                  << std::endl;
        if (recs.empty()) {
            std::cout << "\nRecommendation complete!" << std::endl;
            return true;
        }
    }
    std::cout << "\nTop " << recs.size() << " Recommendations:\n" << std::endl;
    for (size_t i = 0; i < recs.size(); ++i) {
        std::ostringstream value;
        if (nearest) value << "  (" << (o.jaccard ? "similarity " : o.euclidean || o.manhattan ? "distance " : "score ") << values[i] << ")";
        if (o.anyOf && i < matched.size()) value << "  (matches \"" << catalogue.trackNames[static_cast<size_t>(matched[i])] << "\")";
        if (!printEntry(catalogue, genreMap, recs[i], i + 1, "", value.str())) return false;
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
    if (mode == "--song" || mode == "--id" || mode == "--playlist") {
        if (argc < 3 && mode == "--playlist") {
            std::cerr << "Error: --playlist needs a comma-separated list of track IDs" << std::endl;
            return 1;
        }
        if (argc < 3) {
            std::cerr << "Error: Song name or track ID required" << std::endl;
            usage(argv[0]);
            return 1;
        }
        Options o;
        return parseOptions(argc, argv, o) && queryMode(o) ? 0 : 1;
    }
    std::cerr << "Error: Unknown mode '" << mode << "'" << std::endl;
    usage(argv[0]);
    return 1;
}
