// rows_update.h — the host-only part of IN-PLACE ROW UPDATES (include/mi355rec_diag.h, "ROW UPDATES"): what is checked before
// anything is written, and how a node handle deals a list of global rows over its shards.  No HIP in here: the single handle
// (engine_update.hip.h), the node handle (sharded.hip), the CPU backend (cpu_backend.cpp) and tests/update_rows_check.cpp
// (a stand-alone program, built with the host sanitizers) all include it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mi355update {

constexpr int64_t kStageRows = 65536;   // rows of one staged chunk: a larger update goes in several

// What is wrong with rows[0..count) as the rows of one update of a catalogue of n rows, or nothing (0):
//   - a row outside [0, n): every list is refused that names one, before anything is written;
//   - a row named twice: two threads of one launch would race on its entries.
// *at = the position of the first offender in the list (of a duplicate: its SECOND occurrence in list order is not
// promised, only one of the pair).  May throw std::bad_alloc (the callers sit behind a C-ABI and catch it).
enum Bad { kFine = 0, kOutOfRange = 1, kDuplicate = 2 };

inline Bad check_rows(const int64_t* rows, int64_t count, int64_t n, int64_t* at) {
    for (int64_t i = 0; i < count; ++i)
        if (rows[i] < 0 || rows[i] >= n) {
            if (at) *at = i;
            return kOutOfRange;
        }
    if (count < 2) return kFine;
    if (count >= n / 1024) {   // one bit per row of the catalogue (n / 8 bytes to clear) beats a sort unless the list is tiny beside it
        std::vector<uint64_t> seen(static_cast<size_t>((n + 63) / 64), 0);
        for (int64_t i = 0; i < count; ++i) {
            uint64_t& w = seen[static_cast<size_t>(rows[i] >> 6)];
            const uint64_t bit = 1ull << (rows[i] & 63);
            if (w & bit) {
                if (at) *at = i;
                return kDuplicate;
            }
            w |= bit;
        }
        return kFine;
    }
    std::vector<int64_t> order(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) order[static_cast<size_t>(i)] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rows[a] != rows[b] ? rows[a] < rows[b] : a < b; });
    for (int64_t i = 1; i < count; ++i)
        if (rows[order[static_cast<size_t>(i)]] == rows[order[static_cast<size_t>(i - 1)]]) {
            if (at) *at = order[static_cast<size_t>(i)];
            return kDuplicate;
        }
    return kFine;
}

// The message of a refused list (the C-ABI's last-error text).
inline void describe(Bad bad, const int64_t* rows, int64_t at, int64_t n, char* why, size_t why_size) {
    if (bad == kOutOfRange)
        std::snprintf(why, why_size, "row %lld (entry %lld of the update) is outside [0, %lld)", (long long)rows[at], (long long)at, (long long)n);
    else if (bad == kDuplicate)
        std::snprintf(why, why_size, "row %lld is named twice in one update (entry %lld)", (long long)rows[at], (long long)at);
    else if (why_size)
        why[0] = 0;
}

// Balanced contiguous blocks, as the node handle places its shards: the first n % g shards hold one row more.
inline void shard_bounds(int64_t n, int g, int r, int64_t& lo, int64_t& hi) {
    const int64_t per = n / g, rem = n % g;
    lo = r * per + (r < rem ? r : rem);
    hi = lo + per + (r < rem ? 1 : 0);
}

// The part of an update that one shard owns: its rows made LOCAL, and where each stood in the caller's list (its features are
// row at[i] of the caller's matrix).  List order is kept inside a shard.
struct ShardPart {
    std::vector<int64_t> local;
    std::vector<int64_t> at;
};

// Deals rows[0..count) (checked: all inside [0, n)) over g adjacent shards, shard r starting at row lo[r] (ascending; an empty
// shard shares its lo with the next one, or starts at n, and is dealt nothing).  parts is resized to g.  May throw std::bad_alloc.
inline void split_by_shard(const int64_t* rows, int64_t count, const int64_t* lo, int g, std::vector<ShardPart>& parts) {
    parts.assign(static_cast<size_t>(g), ShardPart());
    // the last shard whose first row is <= the row (the empty shards before it share its lo and own nothing)
    auto owner = [&](int64_t row) {
        int a = 0, b = g - 1;
        while (a < b) {
            const int m = (a + b + 1) / 2;
            if (lo[m] <= row) a = m; else b = m - 1;
        }
        return a;
    };
    std::vector<int64_t> fill(static_cast<size_t>(g), 0);   // two passes: count, then place (no vector grows element by element)
    std::vector<int32_t> own(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) {
        own[static_cast<size_t>(i)] = owner(rows[i]);
        ++fill[static_cast<size_t>(own[static_cast<size_t>(i)])];
    }
    for (int r = 0; r < g; ++r) {
        parts[static_cast<size_t>(r)].local.resize(static_cast<size_t>(fill[static_cast<size_t>(r)]));
        parts[static_cast<size_t>(r)].at.resize(static_cast<size_t>(fill[static_cast<size_t>(r)]));
        fill[static_cast<size_t>(r)] = 0;
    }
    for (int64_t i = 0; i < count; ++i) {
        const int a = own[static_cast<size_t>(i)];
        ShardPart& p = parts[static_cast<size_t>(a)];
        const size_t k = static_cast<size_t>(fill[static_cast<size_t>(a)]++);
        p.local[k] = rows[i] - lo[a];
        p.at[k] = i;
    }
}

}  // namespace mi355update
