// shard_merge_check.cpp — a stand-alone program over csrc/shard_merge.h (the host merge of a row-sharded node handle: the leading
// keys of every shard's list, each key's tag with it, the shards' totals summed), built and run by tests/test_shard_merge_cpu.py as
// its own process, with -fsanitize=address,undefined.  The accumulator is compared with a full descending sort of all keys; every
// output buffer is sized exactly, so a write past the answer shows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <utility>
#include <vector>

#include "shard_merge.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// A key as the library packs one: the score's ordered bits above, the row id below so that the LOWER row makes the LARGER key.
static uint64_t key(uint32_t score_bits, uint32_t row) { return (static_cast<uint64_t>(score_bits) << 32) | (0xffffffffu - row); }
static uint32_t row_of(uint64_t k) { return 0xffffffffu - static_cast<uint32_t>(k); }

struct List {
    std::vector<uint64_t> keys;
    int64_t total = 0;
};

static int g_cases = 0;

// Every list into one accumulator (tagged: each key with a tag of its own, never 0), then finish(topn) against the sorted whole.
static int merged_is_the_sorted_whole(const std::vector<List>& lists, int topn, bool tagged) {
    ++g_cases;
    mi355merge::TopKeys merge;
    std::vector<std::pair<uint64_t, int32_t>> all;
    int64_t total = 0;
    int32_t next_tag = 1;
    size_t n_keys = 0;
    for (const List& l : lists) n_keys += l.keys.size();
    merge.reserve(n_keys);
    for (const List& l : lists) {
        std::vector<int32_t> tags;
        for (uint64_t k : l.keys) {
            tags.push_back(next_tag);
            all.emplace_back(k, tagged ? next_tag : 0);
            next_tag += 3;
        }
        merge.add(l.keys.data(), tagged ? tags.data() : nullptr, static_cast<int>(l.keys.size()), l.total);
        total += l.total;
    }
    std::sort(all.begin(), all.end(), [](const std::pair<uint64_t, int32_t>& a, const std::pair<uint64_t, int32_t>& b) { return a.first > b.first; });
    const size_t want = std::min(all.size(), static_cast<size_t>(topn));
    std::vector<uint64_t> out_keys(want);
    std::vector<int32_t> out_tags(tagged ? want : 0);
    const int count = merge.finish(topn, want ? out_keys.data() : nullptr, tagged && want ? out_tags.data() : nullptr);
    CHECK(count == static_cast<int>(want));
    CHECK(merge.total == total);
    for (size_t i = 0; i < want; ++i) {
        CHECK(out_keys[i] == all[i].first);
        if (tagged) CHECK(out_tags[i] == all[i].second);
        if (i > 0) CHECK(out_keys[i - 1] > out_keys[i]);
    }
    return 0;
}

static int both_ways(const std::vector<List>& lists, int topn) {
    if (merged_is_the_sorted_whole(lists, topn, false)) return 1;
    return merged_is_the_sorted_whole(lists, topn, true);
}

int main() {
    const std::vector<int> topns = {0, 1, 3, 10, 1024};
    // every list empty: 1, 3 and 64 of them, with and without totals
    for (int g : {1, 3, 64})
        for (int topn : topns) {
            std::vector<List> lists(static_cast<size_t>(g));
            if (both_ways(lists, topn)) return 1;
            for (int s = 0; s < g; s += 2) lists[static_cast<size_t>(s)].total = 5 + s;   // (a count-only call: no key, a total)
            if (both_ways(lists, topn)) return 1;
        }
    {   // one list supplies the whole answer (the others rank below all of it, or are empty)
        std::vector<List> lists(4);
        for (uint32_t i = 0; i < 8; ++i) lists[2].keys.push_back(key(900 - i, 200 + i));
        for (uint32_t i = 0; i < 5; ++i) lists[0].keys.push_back(key(100 - i, i));
        for (uint32_t i = 0; i < 3; ++i) lists[3].keys.push_back(key(50 - i, 300 + i));
        for (int topn : {1, 8}) if (both_ways(lists, topn)) return 1;
        // ... all of one list and part of another; then fewer keys than topn
        for (int topn : {9, 11, 15, 16, 17, 1024}) if (both_ways(lists, topn)) return 1;
    }
    {   // equal score bits in different lists: the lower row id first, whichever list came first
        for (int order = 0; order < 2; ++order) {
            std::vector<List> lists(3);
            List& early = lists[order ? 2 : 0];
            List& late = lists[order ? 0 : 2];
            early.keys = {key(700, 4), key(500, 9), key(300, 11)};
            late.keys = {key(700, 90), key(500, 80), key(300, 70)};
            lists[1].keys = {key(700, 40), key(600, 41)};
            for (int topn : {1, 2, 3, 4, 5, 8, 1024}) if (both_ways(lists, topn)) return 1;
            mi355merge::TopKeys merge;
            for (const List& l : lists) merge.add(l.keys.data(), nullptr, static_cast<int>(l.keys.size()));
            uint64_t out[8];
            CHECK(merge.finish(8, out) == 8);
            const uint32_t rows[8] = {4, 40, 90, 41, 9, 80, 11, 70};
            for (int i = 0; i < 8; ++i) CHECK(row_of(out[i]) == rows[i]);
        }
    }
    {   // totals: empty addends, addends of lists with and without keys, topn == 0 with a total that stands
        std::vector<List> lists(5);
        lists[0].total = 0;
        lists[1].keys = {key(10, 1), key(9, 2)};
        lists[1].total = 7;
        lists[2].total = 1000000000000ll;   // (beyond int32: the sum is an int64)
        lists[3].keys = {key(11, 3)};
        lists[4].total = 3;
        for (int topn : topns) if (both_ways(lists, topn)) return 1;
        mi355merge::TopKeys merge;
        for (const List& l : lists) merge.add(l.keys.data(), nullptr, static_cast<int>(l.keys.size()), l.total);
        CHECK(merge.finish(0, nullptr) == 0 && merge.total == 1000000000010ll);
    }
    // up to 64 lists of 0 to 8 keys, each list descending as a shard's is, scores from a small range so that they collide
    std::mt19937 rng(2586);
    for (int round = 0; round < 24; ++round) {
        const int g = round < 4 ? 64 : 1 + static_cast<int>(rng() % 64);
        std::vector<List> lists(static_cast<size_t>(g));
        uint32_t row = 0;
        for (List& l : lists) {
            const int n = static_cast<int>(rng() % 9);
            for (int i = 0; i < n; ++i) l.keys.push_back(key(1 + rng() % 12, row++));
            std::sort(l.keys.begin(), l.keys.end(), std::greater<uint64_t>());
            l.total = rng() % 3 ? static_cast<int64_t>(rng() % 1000) : 0;
            row += rng() % 3;
        }
        for (int topn : {1, 7, 1024}) if (both_ways(lists, topn)) return 1;
    }
    std::printf("shard_merge.h: ok (%d cases)\n", g_cases);
    return 0;
}
