// embed_sets_request.h — what libmi355rec_embed_sets.so (include/mi355rec_embed_sets.h) adds to embed_request.h on the
// host: the bitmap of a row set as the scan reads it (bit i of a uint32 word array is local row i = global id - row_base;
// the bits of the last word past row n are zero, and zero words pad the array to a whole number of the largest tile's 32
// words, so a tile-granular read never leaves the allocation), its builder from ids and from a mask, the predicates that
// answer a request without a launch, and the reader of the self-sized ext.  A request is embed_request.h's Request,
// unchanged.  Host code only: no HIP header (tests/embed_sets_check.cpp compiles it with g++).
#pragma once

#include <utility>
#include <vector>

#include "embed_half_request.h"
#include "mi355rec_embed_sets.h"

namespace mi355embedsets {

constexpr int64_t kTileWordsMax = 32;   // the words of the widest tile (1024 rows: half storage at d = 16)

inline int64_t row_words(int64_t n) { return (n + 31) / 32; }
// The words of a bitmap over n rows as it is allocated, on the host and on the device (at least one tile's).
inline int64_t padded_words(int64_t n) {
    const int64_t tiles = (row_words(n) + kTileWordsMax - 1) / kTileWordsMax;
    return (tiles > 0 ? tiles : 1) * kTileWordsMax;
}

struct Bitmap {
    int64_t base = 0, n = 0, count = 0;
    int64_t lo = 0, hi = -1;    // the words that hold a bit, inclusive (hi < lo: none does)
    std::vector<uint32_t> w;    // padded_words(n) words

    void reset(int64_t base_, int64_t n_) {
        base = base_;
        n = n_;
        count = 0;
        lo = 0;
        hi = -1;
        w.assign(static_cast<size_t>(padded_words(n_)), 0u);
    }
    bool test(int64_t row) const { return row >= 0 && row < n && ((w[static_cast<size_t>(row >> 5)] >> (row & 31)) & 1u) != 0u; }
};

// True when the id list cannot be used (the rules of mi355rec_rowset_*); then msg[0..cap) says why.
inline bool invalid_ids(const int64_t* ids, int64_t n_ids, char* msg, size_t cap) {
    if (n_ids < 0) {
        std::snprintf(msg, cap, "row set: n_ids must not be negative, got %lld", static_cast<long long>(n_ids));
        return true;
    }
    if (n_ids > 0 && !ids) {
        std::snprintf(msg, cap, "row set: null id list with n_ids %lld", static_cast<long long>(n_ids));
        return true;
    }
    for (int64_t i = 0; i < n_ids; ++i)
        if (ids[i] < 0) {
            std::snprintf(msg, cap, "row set: negative id %lld", static_cast<long long>(ids[i]));
            return true;
        }
    return false;
}

// What an add changed: (word index, its value before), in the order of the change; undo() puts them back.
using Undo = std::vector<std::pair<int64_t, uint32_t>>;

// The ids into the bitmap.  False (and nothing changed): the list is invalid, msg says why.  With `undo`, the words that
// changed are recorded (the caller puts them back if its upload fails); *w_lo .. *w_hi: the words to upload (hi < lo: none).
inline bool add_ids(Bitmap& b, const int64_t* ids, int64_t n_ids, Undo* undo, int64_t* w_lo, int64_t* w_hi, char* msg, size_t cap) {
    *w_lo = 0;
    *w_hi = -1;
    if (invalid_ids(ids, n_ids, msg, cap)) return false;
    for (int64_t i = 0; i < n_ids; ++i) {
        const int64_t r = ids[i] - b.base;
        if (r < 0 || r >= b.n) continue;   // (ids of other shards match nothing)
        const int64_t wi = r >> 5;
        const uint32_t bit = 1u << (r & 31);
        uint32_t& word = b.w[static_cast<size_t>(wi)];
        if (word & bit) continue;
        if (undo) undo->emplace_back(wi, word);
        word |= bit;
        ++b.count;
        if (*w_hi < *w_lo) *w_lo = *w_hi = wi;
        if (wi < *w_lo) *w_lo = wi;
        if (wi > *w_hi) *w_hi = wi;
    }
    if (*w_hi >= *w_lo) {
        if (b.hi < b.lo) b.lo = *w_lo, b.hi = *w_hi;
        if (*w_lo < b.lo) b.lo = *w_lo;
        if (*w_hi > b.hi) b.hi = *w_hi;
    }
    return true;
}

// Puts back what add_ids recorded (count and the word range are those of `before`).
inline void undo_add(Bitmap& b, const Undo& undo, int64_t count_before, int64_t lo_before, int64_t hi_before) {
    for (size_t i = undo.size(); i-- > 0;) b.w[static_cast<size_t>(undo[i].first)] = undo[i].second;
    b.count = count_before;
    b.lo = lo_before;
    b.hi = hi_before;
}

// mask: n bytes, one per row; non-zero means in the set.  False: the mask cannot be used, msg says why.
inline bool from_mask(Bitmap& b, const uint8_t* mask, int64_t n, char* msg, size_t cap) {
    if (n != b.n) {
        std::snprintf(msg, cap, "row set: mask of %lld bytes for a table of %lld rows", static_cast<long long>(n), static_cast<long long>(b.n));
        return false;
    }
    if (n > 0 && !mask) {
        std::snprintf(msg, cap, "row set: null mask");
        return false;
    }
    for (int64_t r = 0; r < n; ++r) {
        if (!mask[r]) continue;
        const int64_t wi = r >> 5;
        b.w[static_cast<size_t>(wi)] |= 1u << (r & 31);
        ++b.count;
        if (b.hi < b.lo) b.lo = wi;
        b.hi = wi;
    }
    return true;
}

// The word the scan tests a row against: only AND NOT seen (an absent only reads as all ones, an absent seen as zero).
inline uint32_t effective_word(const Bitmap* seen, const Bitmap* only, int64_t wi) {
    const uint32_t o = only ? only->w[static_cast<size_t>(wi)] : ~0u;
    const uint32_t s = seen ? seen->w[static_cast<size_t>(wi)] : 0u;
    return o & ~s;
}

// True when the host bitmaps show that no row is admissible: only is empty, seen holds every row, or only is a subset of
// seen (looked for only where the counts allow it, over the words of only that hold a bit).
inline bool answers_nothing(const Bitmap* seen, const Bitmap* only) {
    if (only && only->count == 0) return true;
    if (seen && seen->count == seen->n) return true;
    if (!seen || !only || only->count > seen->count) return false;
    for (int64_t wi = only->lo; wi <= only->hi; ++wi)
        if (effective_word(seen, only, wi)) return false;
    return true;
}

// The ext as the library reads it (null: no sets), by read_sized' rule.  True when it cannot be used; msg says why.
inline bool read_ext(const mi355rec_embed_sets_ext_t* ext, mi355rec_embed_sets_ext_t* full, char* msg, size_t cap) {
    using E = mi355rec_embed_sets_ext_t;
    std::memset(full, 0, sizeof *full);
    if (!ext) return false;
    static const size_t ends[] = {offsetof(E, flags), offsetof(E, seen), offsetof(E, only), sizeof(E)};
    static_assert(sizeof(E) == offsetof(E, only) + sizeof(void*) && sizeof(E) == 24, "no tail padding: the struct ends where its last field ends");
    if (mi355playlist::read_sized(ext, "embed sets ext", ends, full, msg, cap)) return true;
    if (full->flags != 0u) {
        std::snprintf(msg, cap, "flags 0x%x in an embed sets ext: must be 0", static_cast<unsigned>(full->flags));
        return true;
    }
    return false;
}

}  // namespace mi355embedsets
