// update_rows_check.cpp — csrc/rows_update.h on its own, as a program (tests/test_update_rows_cpu.py builds it with
// -fsanitize=address,undefined and runs it): the checks of an update's row list and the split of a list over shards.
// Prints "rows_update.h: ok" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "rows_update.h"

using namespace mi355update;

static int g_failed = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

static Bad check(const std::vector<int64_t>& rows, int64_t n, int64_t* at = nullptr) {
    int64_t where = -1;
    const Bad b = check_rows(rows.data(), static_cast<int64_t>(rows.size()), n, &where);
    if (at) *at = where;
    return b;
}

static void lists() {
    int64_t at = -1;
    EXPECT(check({}, 10) == kFine);                       // empty lists, and an empty catalogue
    EXPECT(check({}, 0) == kFine);
    EXPECT(check_rows(nullptr, 0, 5, nullptr) == kFine);
    EXPECT(check({0}, 0, &at) == kOutOfRange && at == 0);
    EXPECT(check({0}, 1) == kFine);
    EXPECT(check({9, 0, 5}, 10) == kFine);
    EXPECT(check({9, 0, 10}, 10, &at) == kOutOfRange && at == 2);      // an id equal to n
    EXPECT(check({-1, 0}, 10, &at) == kOutOfRange && at == 0);         // a negative id
    EXPECT(check({3, 3, 11}, 10, &at) == kOutOfRange && at == 2);      // the range is checked before duplicates
    // duplicates at both ends of a list, through the sort (a sparse list) and through the bitmap (a dense one)
    for (int64_t n : {int64_t(50), int64_t(100000000)}) {
        std::vector<int64_t> rows(40);
        std::iota(rows.begin(), rows.end(), 5);
        EXPECT(check(rows, n) == kFine);
        rows.back() = rows.front();
        EXPECT(check(rows, n, &at) == kDuplicate && (at == 0 || at == 39));
        rows.back() = 49;
        rows[1] = rows[0];
        EXPECT(check(rows, n, &at) == kDuplicate && (at == 0 || at == 1));
        rows[1] = 6;
        rows[38] = 49;
        EXPECT(check(rows, n, &at) == kDuplicate && (at == 38 || at == 39));
    }
    std::vector<int64_t> all(100000);
    std::iota(all.begin(), all.end(), 0);
    EXPECT(check(all, 100000) == kFine);                  // every row once, the last bit of the bitmap included
    all[0] = 99999;
    EXPECT(check(all, 100000, &at) == kDuplicate && at == 99999);
    char why[160];
    const std::vector<int64_t> bad = {4, 7, 4};
    const Bad what = check(bad, 10, &at);
    describe(what, bad.data(), at, 10, why, sizeof why);
    EXPECT(why[0] != 0);
    describe(kFine, bad.data(), 0, 10, why, sizeof why);
    EXPECT(why[0] == 0);
}

// Every id goes to the shard that owns it, is made local, keeps its place in the caller's list, and nothing is lost.
static void split_case(const std::vector<int64_t>& rows, int64_t n, int g) {
    std::vector<int64_t> lo(static_cast<size_t>(g)), hi(static_cast<size_t>(g));
    for (int r = 0; r < g; ++r) shard_bounds(n, g, r, lo[static_cast<size_t>(r)], hi[static_cast<size_t>(r)]);
    EXPECT(lo[0] == 0 && hi[static_cast<size_t>(g) - 1] == n);
    std::vector<ShardPart> parts;
    split_by_shard(rows.data(), static_cast<int64_t>(rows.size()), lo.data(), g, parts);
    EXPECT(parts.size() == static_cast<size_t>(g));
    size_t total = 0;
    std::vector<char> seen(rows.size(), 0);
    const int64_t* all = rows.data();
    const int64_t count = static_cast<int64_t>(rows.size());
    char* mark = seen.data();
    for (int r = 0; r < g; ++r) {
        const ShardPart& p = parts[static_cast<size_t>(r)];
        EXPECT(p.local.size() == p.at.size());
        if (p.local.size() != p.at.size()) continue;
        total += p.local.size();
        const int64_t first = lo[static_cast<size_t>(r)], width = hi[static_cast<size_t>(r)] - first;
        const int64_t *local = p.local.data(), *where = p.at.data();
        bool in_list = true, once = true, inside = true, same = true, ordered = true;
        for (size_t i = 0; i < p.local.size(); ++i) {
            const int64_t at = where[i];
            if (at < 0 || at >= count) {
                in_list = false;
                continue;
            }
            once = once && !mark[at];
            mark[at] = 1;
            inside = inside && local[i] >= 0 && local[i] < width;
            same = same && local[i] + first == all[at];
            ordered = ordered && (i == 0 || where[i - 1] < at);   // list order is kept inside a shard
        }
        EXPECT(in_list);
        EXPECT(once);
        EXPECT(inside);
        EXPECT(same);
        EXPECT(ordered);
    }
    EXPECT(total == rows.size());
}

static void splits() {
    // 10^6 ids of a 10^7-row catalogue: a multiplicative walk, so neither sorted nor clustered
    std::vector<int64_t> many(1000000);
    for (size_t i = 0; i < many.size(); ++i) many[i] = static_cast<int64_t>((i * 7919ull + 13ull) % 10000000ull);
    for (int g = 1; g <= 64; ++g) {
        split_case({}, 1000, g);
        for (int64_t n : {int64_t(1), int64_t(9), int64_t(63), int64_t(4097)}) {   // fewer rows than shards: empty shards at the end
            std::vector<int64_t> edges;                   // ids at every shard edge: the last row of a shard and the first of the next
            for (int r = 0; r < g; ++r) {
                int64_t lo, hi;
                shard_bounds(n, g, r, lo, hi);
                if (hi > lo) {
                    edges.push_back(hi - 1);
                    if (hi - 1 != lo) edges.push_back(lo);
                }
            }
            split_case(edges, n, g);
        }
        split_case(many, 10000000, g);
    }
}

int main() {
    lists();
    splits();
    if (g_failed) {
        std::printf("rows_update.h: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("rows_update.h: ok\n");
    return 0;
}
