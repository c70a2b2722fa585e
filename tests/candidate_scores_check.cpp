// candidate_scores_check.cpp — a stand-alone program over csrc/candidates.h's `positions` (CANDIDATE SCORES: from list order to the
// entry of the shard's sorted, distinct list), built and run by tests/test_candidate_scores_cpu.py as its own process with
// -fsanitize=address,undefined.  Every buffer is sized exactly, so a read or write past the list shows.
#include <cstdint>
#include <cstdio>
#include <random>
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

// reduce() then positions() into buffers of exactly ids.size() entries (one where the list is empty): every in-range id finds its own
// local row in the reduced list, every other id -1; every entry of the reduced list is some id's.
static int positions_find_their_rows(const std::vector<int64_t>& ids, int64_t lo, int64_t hi, bool want_ascending) {
    const int64_t n = static_cast<int64_t>(ids.size());
    std::vector<uint32_t> rows(ids.empty() ? 1 : ids.size());
    std::vector<int64_t> pos(ids.empty() ? 1 : ids.size(), -7);
    const Reduced r = mi355cand::reduce(ids.data(), n, lo, hi, rows.data());
    CHECK(r.ascending == want_ascending);
    mi355cand::positions(ids.data(), n, lo, hi, rows.data(), r, pos.data());
    std::vector<char> used(static_cast<size_t>(r.count) + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[static_cast<size_t>(i)], p = pos[static_cast<size_t>(i)];
        if (id < lo || id >= hi) {
            CHECK(p == -1);
            continue;
        }
        CHECK(p >= 0 && p < r.count && static_cast<int64_t>(rows[static_cast<size_t>(p)]) == id - lo);
        used[static_cast<size_t>(p)] = 1;
    }
    for (int64_t e = 0; e < r.count; ++e) CHECK(used[static_cast<size_t>(e)]);
    if (ids.empty()) CHECK(pos[0] == -7);   // nothing is written for an empty list
    return 0;
}

int main() {
    const int64_t kIdEnd = int64_t(1) << 32;
    // empty, one id inside and outside, ascending (one pass, nothing searched), shuffled, duplicated
    CHECK(!positions_find_their_rows({}, 0, 100, true));
    CHECK(!positions_find_their_rows({42}, 0, 100, true));
    CHECK(!positions_find_their_rows({42}, 43, 100, true));
    CHECK(!positions_find_their_rows({1, 2, 3, 50, 99}, 0, 100, true));
    CHECK(!positions_find_their_rows({99, 50, 3, 2, 1}, 0, 100, false));
    CHECK(!positions_find_their_rows({1, 2, 2, 3}, 0, 100, false));
    CHECK(!positions_find_their_rows({5, 5, 5, 5}, 0, 100, false));
    // ids on both sides of [row_base, row_base + n): -1 for those, and they do not disturb the ascending pass
    CHECK(!positions_find_their_rows({2000, 1000, 1001, 5, 1099, 1100, 999}, 1000, 1100, true));
    CHECK(!positions_find_their_rows({1099, 5, 1000, 4294967295ll, 1099}, 1000, 1100, false));
    CHECK(!positions_find_their_rows({5, 2000, 999, 1100}, 1000, 1100, true));   // no id of the shard at all
    // the ends of the id range
    CHECK(!positions_find_their_rows({kIdEnd - 1, kIdEnd - 100, 0}, kIdEnd - 100, kIdEnd, false));
    CHECK(!positions_find_their_rows({0, kIdEnd - 1}, 0, kIdEnd, true));
    // random lists over shards with lo, hi at 0, 1, n - 1 and n
    std::mt19937_64 rng(21);
    for (int64_t n : {1, 2, 5, 257, 2049}) {
        std::vector<int64_t> ids, sorted;
        for (int i = 0; i < 3 * n + 7; ++i) ids.push_back(static_cast<int64_t>(rng() % static_cast<uint64_t>(n + 3)));
        for (int64_t i = 0; i < n; i += 3) sorted.push_back(i);
        for (int64_t lo : {int64_t(0), int64_t(1), n - 1, n})
            for (int64_t hi : {int64_t(0), int64_t(1), n - 1, n}) {
                if (hi < lo) continue;
                std::vector<uint32_t> rows(ids.size());
                const bool asc = mi355cand::reduce(ids.data(), static_cast<int64_t>(ids.size()), lo, hi, rows.data()).ascending;
                CHECK(!positions_find_their_rows(ids, lo, hi, asc));
                CHECK(!positions_find_their_rows(sorted, lo, hi, true));
            }
    }
    std::printf("candidates.h positions: ok\n");
    return 0;
}
