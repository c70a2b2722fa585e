// shard_merge.h — the host merge of a ROW-SHARDED node handle (sharded.hip, merge_over_shards): every shard answers with its own
// leading keys, and the node's answer is the leading keys of them all.  Keys come PACKED (mi355rec_pack_key: score, then the lower
// row id, in one uint64 that compares as the result order does; packing and unpacking stay with the caller), each with an optional
// int32 tag that travels with it ("ANY-OF REQUESTS": the member index) and each shard with an optional partial total that is summed
// ("BOUNDED REQUESTS": the rows that match).  Pure arithmetic on uint64: exact, whatever the number of shards.
// Host only: no HIP type or call (tests/shard_merge_check.cpp compiles it with g++).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mi355merge {

// Throws std::bad_alloc where the host has no memory left; nothing after reserve(n) does while at most n keys are added.
struct TopKeys {
    std::vector<std::pair<uint64_t, int32_t>> keys;   // (key, tag) of every shard so far; the tag is 0 where none was given
    int64_t total = 0;                                // the partial totals so far

    void reserve(size_t n) { keys.reserve(n); }

    // One shard's answer: n keys, their tags (or null) and its partial total.
    void add(const uint64_t* shard_keys, const int32_t* tags, int n, int64_t partial_total = 0) {
        for (int i = 0; i < n; ++i) keys.emplace_back(shard_keys[i], tags ? tags[i] : 0);
        total += partial_total;
    }

    // The leading min(topn, keys) keys, largest first (an equal score: the lower row id, as the key encodes), to out_keys and, where
    // it is given, their tags to out_tags.  Returns how many.  topn == 0 writes nothing (the buffers may be null); `total` stands.
    int finish(int topn, uint64_t* out_keys, int32_t* out_tags = nullptr) {
        const size_t count = std::min(keys.size(), static_cast<size_t>(topn));
        std::partial_sort(keys.begin(), keys.begin() + count, keys.end(),
                          [](const std::pair<uint64_t, int32_t>& a, const std::pair<uint64_t, int32_t>& b) { return a.first > b.first; });
        for (size_t i = 0; i < count; ++i) {
            out_keys[i] = keys[i].first;
            if (out_tags) out_tags[i] = keys[i].second;
        }
        return static_cast<int>(count);
    }
};

}  // namespace mi355merge
