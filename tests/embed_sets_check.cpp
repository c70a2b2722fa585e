// embed_sets_check.cpp — csrc/embed_sets_request.h as a stand-alone program (its own main), built by
// tests/test_embed_sets_cpu.py with -fsanitize=address,undefined: ids and masks into bits (duplicates, ids outside the rows,
// a row base), add and a failed add, the count, the zero tail of the last word and the zero padding to 32 words, the
// no-launch predicates, and the ext read from a heap buffer of exactly its size, as the library reads it.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "embed_sets_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using namespace mi355embedsets;

int64_t popcount_all(const Bitmap& b) {
    int64_t c = 0;
    for (uint32_t w : b.w) c += __builtin_popcount(w);
    return c;
}

bool add(Bitmap& b, const std::vector<int64_t>& ids, int64_t* lo = nullptr, int64_t* hi = nullptr) {
    char msg[256];
    int64_t l, h;
    const bool ok = add_ids(b, ids.data(), static_cast<int64_t>(ids.size()), nullptr, &l, &h, msg, sizeof msg);
    if (lo) *lo = l;
    if (hi) *hi = h;
    return ok;
}

void check_sizes() {
    EXPECT(padded_words(0) == 32 && padded_words(1) == 32 && padded_words(1024) == 32 && padded_words(1025) == 64);
    EXPECT(padded_words(65537) == 2080 && padded_words(1000003) % 32 == 0 && padded_words(1000003) * 32 >= 1000003);
    // every tile of every layout (64 .. 1024 rows, a divisor of 1024) reads whole words inside the allocation
    for (int64_t n : {1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097, 65537})
        for (int64_t tile_rows : {64, 128, 256, 512, 1024}) {
            const int64_t n_tiles = (n + tile_rows - 1) / tile_rows;
            EXPECT(n_tiles * (tile_rows / 32) <= padded_words(n));
        }
}

void check_ids() {
    for (int64_t base : {int64_t{0}, int64_t{1000000}}) {
        for (int64_t n : {1, 2, 31, 32, 33, 63, 64, 65, 1025, 4097}) {
            Bitmap b;
            b.reset(base, n);
            EXPECT(static_cast<int64_t>(b.w.size()) == padded_words(n) && b.count == 0 && b.hi < b.lo);
            // duplicates in any order, the first and the last row, ids below, above and far outside the rows
            std::vector<int64_t> ids = {base + n - 1, base, base, base + n, base + n + 31, base + n - 1, int64_t{1} << 40};
            if (base > 0) ids.insert(ids.end(), {base - 1, 0, n - 1});
            int64_t lo, hi;
            EXPECT(add(b, ids, &lo, &hi));
            const int64_t want = n == 1 ? 1 : 2;
            EXPECT(b.count == want && popcount_all(b) == want);
            EXPECT(b.test(0) && b.test(n - 1) && !b.test(n) && !b.test(-1));
            EXPECT(lo == 0 && hi == (n - 1) / 32 && b.lo == 0 && b.hi == (n - 1) / 32);
            // the tail of the last word and the padding words are zero
            const int64_t last = (n - 1) / 32;
            if (n % 32) EXPECT((b.w[static_cast<size_t>(last)] >> (n % 32)) == 0u);
            for (size_t w = static_cast<size_t>(last) + 1; w < b.w.size(); ++w) EXPECT(b.w[w] == 0u);
            // an add of what is there changes nothing and asks for no upload
            EXPECT(add(b, {base, base + n - 1}, &lo, &hi) && hi < lo && b.count == want);
        }
    }
    // the word edge: rows 31 and 32 alone
    Bitmap b;
    b.reset(0, 100);
    EXPECT(add(b, {31, 32}) && b.w[0] == 0x80000000u && b.w[1] == 1u && b.count == 2 && b.lo == 0 && b.hi == 1);
    EXPECT(add(b, {}) && b.count == 2);   // n_ids == 0 (the list is never read)
}

void check_failed_add() {
    Bitmap b;
    b.reset(10, 70);
    EXPECT(add(b, {10, 45}));
    const std::vector<uint32_t> before = b.w;
    char msg[256];
    int64_t lo, hi;
    const int64_t bad[] = {12, 13, -1, 14};
    Undo undo;
    EXPECT(!add_ids(b, bad, 4, &undo, &lo, &hi, msg, sizeof msg) && std::strstr(msg, "negative id -1"));
    EXPECT(b.w == before && b.count == 2 && undo.empty() && hi < lo);
    EXPECT(!add_ids(b, nullptr, 3, &undo, &lo, &hi, msg, sizeof msg) && std::strstr(msg, "null id list with n_ids 3"));
    EXPECT(!add_ids(b, bad, -2, &undo, &lo, &hi, msg, sizeof msg) && std::strstr(msg, "n_ids must not be negative, got -2"));
    EXPECT(add_ids(b, nullptr, 0, &undo, &lo, &hi, msg, sizeof msg) && b.w == before);
    // an add that the caller takes back (its upload failed): words, count and range are those of before
    const int64_t more[] = {79, 11, 79, 10, 44};
    const int64_t blo = b.lo, bhi = b.hi;
    EXPECT(add_ids(b, more, 5, &undo, &lo, &hi, msg, sizeof msg) && b.count == 5 && undo.size() == 3 && lo == 0 && hi == 2 && b.hi == 2);
    undo_add(b, undo, 2, blo, bhi);
    EXPECT(b.w == before && b.count == 2 && b.lo == blo && b.hi == bhi);
    char tiny[8];
    EXPECT(!add_ids(b, bad, 4, nullptr, &lo, &hi, tiny, sizeof tiny) && tiny[7] == 0);   // a message longer than its buffer
}

void check_mask() {
    char msg[256];
    for (int64_t n : {1, 31, 32, 33, 64, 65, 1027}) {
        std::unique_ptr<uint8_t[]> mask(new uint8_t[n]);   // exactly n bytes
        Bitmap b, want;
        b.reset(5, n);
        want.reset(5, n);
        std::vector<int64_t> ids;
        for (int64_t r = 0; r < n; ++r) {
            mask[r] = (r % 3 == 0 || r == n - 1) ? static_cast<uint8_t>(1 + r % 255) : 0;
            if (mask[r]) ids.push_back(5 + r);
        }
        EXPECT(from_mask(b, mask.get(), n, msg, sizeof msg) && add(want, ids));
        EXPECT(b.w == want.w && b.count == want.count && b.lo == want.lo && b.hi == want.hi);
        Bitmap c;
        c.reset(5, n);
        EXPECT(!from_mask(c, mask.get(), n - 1, msg, sizeof msg) && std::strstr(msg, "mask of"));
        EXPECT(!from_mask(c, nullptr, n, msg, sizeof msg) && std::strstr(msg, "null mask") && c.count == 0);
    }
    Bitmap z;
    z.reset(0, 0);
    EXPECT(from_mask(z, nullptr, 0, msg, sizeof msg) && z.count == 0);
}

void check_no_launch() {
    const int64_t n = 200;
    Bitmap empty, all, evens, some, some_more;
    for (Bitmap* b : {&empty, &all, &evens, &some, &some_more}) b->reset(0, n);
    std::vector<int64_t> every, even;
    for (int64_t r = 0; r < n; ++r) {
        every.push_back(r);
        if (r % 2 == 0) even.push_back(r);
    }
    EXPECT(add(all, every) && add(evens, even) && add(some, {64, 66, 130}) && add(some_more, {64, 66, 130, 131}));
    EXPECT(!answers_nothing(nullptr, nullptr));
    EXPECT(answers_nothing(nullptr, &empty) && !answers_nothing(&empty, nullptr));       // only empty; seen empty
    EXPECT(answers_nothing(&all, nullptr) && !answers_nothing(nullptr, &all));           // seen holds every row
    EXPECT(answers_nothing(&all, &evens) && answers_nothing(&evens, &some));             // only is a subset of seen
    EXPECT(!answers_nothing(&evens, &some_more) && !answers_nothing(&some, &evens));     // row 131 is odd; more rows than seen has
    EXPECT(answers_nothing(&some, &some) && !answers_nothing(&some, &some_more) && answers_nothing(&some_more, &some));
    EXPECT(!answers_nothing(&evens, &all) && answers_nothing(&empty, &empty));
    // the effective word: an absent only reads as all ones, an absent seen as zero
    EXPECT(effective_word(nullptr, nullptr, 0) == ~0u && effective_word(&evens, nullptr, 0) == 0xAAAAAAAAu);
    EXPECT(effective_word(nullptr, &some, 2) == 5u && effective_word(&evens, &some_more, 4) == 8u && effective_word(&all, &all, 1) == 0u);
}

void check_ext() {
    using E = mi355rec_embed_sets_ext_t;
    char msg[256];
    E full;
    EXPECT(!read_ext(nullptr, &full, msg, sizeof msg) && !full.seen && !full.only);
    E ext{};
    ext.size = sizeof ext;
    ext.seen = reinterpret_cast<const mi355rec_embed_sets_rowset_t*>(&ext);
    ext.only = reinterpret_cast<const mi355rec_embed_sets_rowset_t*>(&msg);
    for (size_t size : {size_t{4}, size_t{8}, size_t{16}, size_t{24}}) {   // the end of every field, from a buffer of exactly that size
        std::unique_ptr<unsigned char[]> buf(new unsigned char[size]);
        ext.size = static_cast<uint32_t>(size);
        std::memcpy(buf.get(), &ext, size);
        EXPECT(!read_ext(reinterpret_cast<const E*>(buf.get()), &full, msg, sizeof msg));
        EXPECT((full.seen != nullptr) == (size >= 16) && (full.only != nullptr) == (size >= 24));
    }
    for (uint32_t size : {0u, 6u, 12u, 20u, 32u}) {
        E bad = ext;
        bad.size = size;
        EXPECT(read_ext(&bad, &full, msg, sizeof msg) && std::strstr(msg, "embed sets ext of size"));
    }
    ext.size = sizeof ext;
    ext.flags = 2;
    EXPECT(read_ext(&ext, &full, msg, sizeof msg) && std::strstr(msg, "flags 0x2 in an embed sets ext: must be 0"));
}

}  // namespace

int main() {
    check_sizes();
    check_ids();
    check_failed_add();
    check_mask();
    check_no_launch();
    check_ext();
    if (failures) {
        std::printf("embed_sets_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_sets_request.h: ok\n");
    return 0;
}
