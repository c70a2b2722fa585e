// candidates_check.cpp — a stand-alone program over csrc/candidates.h (CANDIDATE LISTS: the list's checks, its reduction to a shard's
// sorted, distinct local rows, the split over shard ranges, the membership test), built and run by tests/test_candidates_cpu.py as its
// own process, with -fsanitize=address,undefined where that links.  Every buffer is sized exactly, so a write past the list shows.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "candidates.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

using mi355cand::Reduced;

// reduce() into a buffer of exactly ids.size() entries (one where the list is empty), against std::set.
static int reduce_matches_a_set(const std::vector<int64_t>& ids, int64_t lo, int64_t hi, bool want_ascending, bool check_flag) {
    std::vector<uint32_t> out(ids.empty() ? 1 : ids.size());
    const Reduced r = mi355cand::reduce(ids.data(), static_cast<int64_t>(ids.size()), lo, hi, out.data());
    std::set<int64_t> want;
    for (int64_t id : ids)
        if (id >= lo && id < hi) want.insert(id - lo);
    CHECK(r.count == static_cast<int64_t>(want.size()));
    int64_t i = 0;
    for (int64_t row : want) CHECK(out[static_cast<size_t>(i++)] == static_cast<uint32_t>(row));
    if (check_flag) CHECK(r.ascending == want_ascending);
    for (int64_t row = -2; row < hi - lo + 2 && row < 5000; ++row)
        CHECK(mi355cand::contains(out.data(), r.count, row) == (want.count(row) != 0));
    return 0;
}

int main() {
    char msg[160];
    const int64_t kMax = 1 << 20, kIdEnd = int64_t(1) << 32;
    // the list's checks and their messages
    const int64_t good[] = {0, 5, 5, kIdEnd - 1};
    CHECK(!mi355cand::invalid_list(good, 4, kMax, kIdEnd, msg, sizeof msg));
    CHECK(!mi355cand::invalid_list(nullptr, 0, kMax, kIdEnd, msg, sizeof msg));
    CHECK(!mi355cand::invalid_list(good, 0, kMax, kIdEnd, msg, sizeof msg));
    CHECK(mi355cand::invalid_list(nullptr, 3, kMax, kIdEnd, msg, sizeof msg) && !std::strcmp(msg, "candidate list: null list with n_candidates 3"));
    CHECK(mi355cand::invalid_list(good, -1, kMax, kIdEnd, msg, sizeof msg) &&
          !std::strcmp(msg, "candidate list: n_candidates must not be negative, got -1"));
    CHECK(mi355cand::invalid_list(good, kMax + 1, kMax, kIdEnd, msg, sizeof msg) &&   // (refused before an id is read)
          !std::strcmp(msg, "candidate list: n_candidates 1048577 above MI355REC_MAX_CANDIDATES (1048576)"));
    const int64_t neg[] = {3, -7}, big[] = {kIdEnd}, node_big[] = {99, 100};
    CHECK(mi355cand::invalid_list(neg, 2, kMax, kIdEnd, msg, sizeof msg) && std::strstr(msg, "id -7 out of [0, 4294967296)"));
    CHECK(mi355cand::invalid_list(big, 1, kMax, kIdEnd, msg, sizeof msg) && std::strstr(msg, "id 4294967296 out of"));
    CHECK(mi355cand::invalid_list(node_big, 2, kMax, 100, msg, sizeof msg) && std::strstr(msg, "id 100 out of [0, 100)"));
    CHECK(!mi355cand::invalid_list(node_big, 1, kMax, 100, msg, sizeof msg));
    {   // a list of exactly the maximum passes
        std::vector<int64_t> full(static_cast<size_t>(kMax), 7);
        CHECK(!mi355cand::invalid_list(full.data(), kMax, kMax, kIdEnd, msg, sizeof msg));
    }

    // the count's checks alone read no id
    CHECK(!mi355cand::invalid_count(neg, 2, kMax, msg, sizeof msg));
    CHECK(mi355cand::invalid_count(nullptr, 3, kMax, msg, sizeof msg) && mi355cand::invalid_count(good, -1, kMax, msg, sizeof msg) &&
          mi355cand::invalid_count(good, kMax + 1, kMax, msg, sizeof msg));
    {   // the range check inside the reducing pass: the first id outside [0, id_end) stops it, wherever the shard lies
        const int64_t ids[] = {1005, 7, 1001, -3, 1002, kIdEnd};
        uint32_t out[6];
        Reduced r = mi355cand::reduce(ids, 6, 1000, 1100, out, kIdEnd);
        CHECK(r.bad == 3);
        r = mi355cand::reduce(ids, 3, 1000, 1100, out, kIdEnd);
        CHECK(r.bad == -1 && r.count == 2 && out[0] == 1u && out[1] == 5u && !r.ascending);
        r = mi355cand::reduce(ids + 4, 2, 1000, 1100, out, kIdEnd);
        CHECK(r.bad == 1);
        r = mi355cand::reduce(ids + 4, 2, 1000, 1100, out);              // checked already: ids of no row match nothing
        CHECK(r.bad == -1 && r.count == 1 && out[0] == 2u);
        r = mi355cand::reduce(ids, 6, 0, 100, out, 100);                 // a node's id range: 1005 is the first that is outside
        CHECK(r.bad == 0);
        mi355cand::bad_id_message(ids[3], kIdEnd, msg, sizeof msg);
        CHECK(!std::strcmp(msg, "candidate list: id -3 out of [0, 4294967296)"));
    }

    // empty list, one id, ascending (nothing is sorted), descending, duplicates
    CHECK(!reduce_matches_a_set({}, 0, 100, true, true));
    CHECK(!reduce_matches_a_set({42}, 0, 100, true, true));
    CHECK(!reduce_matches_a_set({42}, 43, 100, true, true));
    CHECK(!reduce_matches_a_set({1, 2, 3, 50, 99}, 0, 100, true, true));
    CHECK(!reduce_matches_a_set({99, 50, 3, 2, 1}, 0, 100, false, true));
    CHECK(!reduce_matches_a_set({1, 2, 2, 3}, 0, 100, false, true));   // a repeat is not STRICTLY ascending: sorted and made distinct
    CHECK(!reduce_matches_a_set({5, 5, 5, 5}, 0, 100, false, true));
    // ids on both sides of [row_base, row_base + n): those outside match nothing and do not disturb the ascending test
    CHECK(!reduce_matches_a_set({2000, 1000, 1001, 5, 1099, 1100, 999}, 1000, 1100, true, true));
    CHECK(!reduce_matches_a_set({1099, 5, 1000, 4294967295ll}, 1000, 1100, false, true));
    // the ends of the id range: a shard that ends at 2^32
    CHECK(!reduce_matches_a_set({kIdEnd - 1, kIdEnd - 100, 0}, kIdEnd - 100, kIdEnd, false, true));
    CHECK(!reduce_matches_a_set({0, kIdEnd - 100, kIdEnd - 1}, kIdEnd - 100, kIdEnd, true, true));
    {   // a shard of 2^32 rows: local row 2^32 - 1 fits uint32
        const int64_t ids[] = {0, kIdEnd - 1};
        uint32_t out[2];
        const Reduced r = mi355cand::reduce(ids, 2, 0, kIdEnd, out);
        CHECK(r.count == 2 && r.ascending && out[0] == 0u && out[1] == 0xffffffffu);
        CHECK(mi355cand::contains(out, 2, kIdEnd - 1) && !mi355cand::contains(out, 2, kIdEnd) && !mi355cand::contains(out, 2, -1));
    }

    // the shard split with lo, hi at 0, 1 and n - 1, and random lists against std::set
    std::mt19937_64 rng(19);
    for (int64_t n : {1, 2, 5, 257, 2049}) {
        std::vector<int64_t> ids;
        for (int i = 0; i < 3 * n + 7; ++i) ids.push_back(static_cast<int64_t>(rng() % static_cast<uint64_t>(n)));
        for (int64_t lo : {int64_t(0), int64_t(1), n - 1, n})
            for (int64_t hi : {int64_t(0), int64_t(1), n - 1, n}) {
                if (lo < 0 || hi < lo) continue;
                std::vector<int64_t> part;
                mi355cand::split(ids.data(), static_cast<int64_t>(ids.size()), lo, hi, &part);
                size_t at = 0;
                for (int64_t id : ids)
                    if (id >= lo && id < hi) CHECK(at < part.size() && part[at++] == id);   // the ids of the range, in list order
                CHECK(at == part.size());
                CHECK(!reduce_matches_a_set(part, lo, hi, false, false));
                CHECK(!reduce_matches_a_set(ids, lo, hi, false, false));   // (the shard reduces the whole list to the same rows)
            }
        // the shards' distinct counts add up to the catalogue's
        std::vector<uint32_t> out(ids.size());
        const int64_t whole = mi355cand::reduce(ids.data(), static_cast<int64_t>(ids.size()), 0, n, out.data()).count;
        const int64_t cut = n / 2;
        const int64_t a = mi355cand::reduce(ids.data(), static_cast<int64_t>(ids.size()), 0, cut, out.data()).count;
        const int64_t b = mi355cand::reduce(ids.data(), static_cast<int64_t>(ids.size()), cut, n, out.data()).count;
        CHECK(a + b == whole);
    }
    std::printf("candidates.h: ok\n");
    return 0;
}
