// rowset.h — ROW SETS (include/mi355rec_diag.h, "ROW SETS"): one bit per row, on the host.  The id checks, the bitmap (bit i of a
// uint32 word array is row i: on a little-endian host bit i & 7 of byte i / 8, which is how playlist_scan_kernel reads its copy), the
// slice of a global bitmap for a shard [lo, hi) and the distinct-row counts, shared by the single handle (engine_rowset.hip.h), the
// node handle (sharded.hip) and the CPU backend.  Host only: no HIP type or call (tests/rowset_check.cpp compiles it with g++).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace mi355rowset {

inline size_t words_for(int64_t n_bits) { return static_cast<size_t>((n_bits + 31) / 32); }

inline bool test_bit(const uint32_t* w, int64_t i) { return ((w[i >> 5] >> (i & 31)) & 1u) != 0u; }

// Bits [0, n_bits) of w that are set (bits past n_bits are not looked at).
inline int64_t popcount(const uint32_t* w, int64_t n_bits) {
    int64_t c = 0;
    const int64_t whole = n_bits >> 5;
    for (int64_t i = 0; i < whole; ++i) c += __builtin_popcount(w[i]);
    if (n_bits & 31) c += __builtin_popcount(w[whole] & ((1u << (n_bits & 31)) - 1u));
    return c;
}

// dst bit i = src bit lo + i for i in [0, hi - lo); every later bit of dst's words_for(hi - lo) words is 0.  lo is in general no
// multiple of 8 or 32: a destination word is put together from two source words.  src holds at least words_for(hi) words.
inline void slice(const uint32_t* src, int64_t lo, int64_t hi, uint32_t* dst) {
    const int64_t n = hi > lo ? hi - lo : 0;
    const size_t nw = words_for(n);
    const size_t src_words = words_for(hi);
    const int sh = static_cast<int>(lo & 31);
    for (size_t w = 0; w < nw; ++w) {
        const size_t s = static_cast<size_t>(lo >> 5) + w;
        uint32_t v = src[s] >> sh;
        if (sh && s + 1 < src_words) v |= src[s + 1] << (32 - sh);
        dst[w] = v;
    }
    if (n & 31) dst[nw - 1] &= (1u << (n & 31)) - 1u;
}

// True when the id list cannot be used: n_ids < 0, a null list with n_ids > 0, or an id outside [0, id_end); msg[0..cap) says why
// and names the id.
inline bool invalid_ids(const int64_t* ids, int64_t n_ids, int64_t id_end, char* msg, size_t cap) {
    if (n_ids < 0) {
        std::snprintf(msg, cap, "row set: n_ids must not be negative, got %lld", static_cast<long long>(n_ids));
        return true;
    }
    if (n_ids > 0 && !ids) {
        std::snprintf(msg, cap, "row set: null id list with n_ids %lld", static_cast<long long>(n_ids));
        return true;
    }
    for (int64_t i = 0; i < n_ids; ++i)
        if (ids[i] < 0 || ids[i] >= id_end) {
            std::snprintf(msg, cap, "row set: id %lld out of [0, %lld)", static_cast<long long>(ids[i]), static_cast<long long>(id_end));
            return true;
        }
    return false;
}

// Rows [base, base + n) of some id space as a bitmap: bit i is row base + i.  count: the distinct rows set.
struct Bitmap {
    int64_t base = 0, n = 0, count = 0;
    std::vector<uint32_t> w;   // words_for(n) words (at least one), padding bits 0

    void reset(int64_t base_, int64_t n_) {
        base = base_;
        n = n_;
        count = 0;
        w.assign(words_for(n_) ? words_for(n_) : 1, 0u);
    }
    // Checked ids (invalid_ids); ids outside [base, base + n) match nothing, duplicates count once.
    void add(const int64_t* ids, int64_t n_ids) {
        for (int64_t i = 0; i < n_ids; ++i) {
            const int64_t r = ids[i] - base;
            if (r < 0 || r >= n) continue;
            const uint32_t bit = 1u << (r & 31);
            uint32_t& word = w[static_cast<size_t>(r >> 5)];
            count += (word & bit) ? 0 : 1;
            word |= bit;
        }
    }
    bool test(int64_t row) const { return row >= 0 && row < n && test_bit(w.data(), row); }
};

// One copy of (a slice of) the set beside the rows that a scan reads: rows [lo, hi) of the set's bitmap, for the engine whose rows
// live at `rows_key` (a handle and its lanes share them).  d_bits: words_for(hi - lo) words on `device` (at least one), padding 0.
struct Part {
    const void* rows_key = nullptr;
    int device = 0;
    int64_t lo = 0, hi = 0;
    int64_t count = 0;         // distinct rows of [lo, hi) in the set
    uint8_t* d_bits = nullptr;
};

}  // namespace mi355rowset

struct mi355rec_sharded;

// The C-ABI's set.  `node`: the node handle it was made on (then bits are global rows), or null: made on a single handle, whose rows
// are `parts[0].rows_key` (then bits are that handle's local rows, base = its row_base).  A CPU-backend node has no parts.
struct mi355rec_rowset {
    const mi355rec_sharded* node = nullptr;
    mi355rowset::Bitmap bits;
    std::vector<mi355rowset::Part> parts;
};

namespace mi355rowset {

// Is `row` of the set's id space admissible for a request that carries the set (null: every row is)?
inline bool admits(const mi355rec_rowset* s, bool only, int64_t row) { return !s || s->bits.test(row) == only; }

}  // namespace mi355rowset
