// rowset_check.cpp — a stand-alone program over csrc/rowset.h (ROW SETS: the host bitmap), built and run by tests/test_rowset_cpu.py
// as its own process, with -fsanitize=address,undefined where that links.
//   rowset_check                     the self-checks below: set / test / count, the id checks, slices against a bit-by-bit loop
//   rowset_check slice IN OUT        IN: int64 n_bits, int64 n_pairs, uint32 words[words_for(n_bits)], int64 (lo, hi)[n_pairs];
//                                    OUT: per pair the words_for(hi - lo) words of slice() and, as one int64, their popcount
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rowset.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int self_checks() {
    using namespace mi355rowset;
    char msg[160];
    // the id checks
    const int64_t good[] = {0, 5, 5, 99};
    CHECK(!invalid_ids(good, 4, 100, msg, sizeof msg));
    CHECK(!invalid_ids(nullptr, 0, 100, msg, sizeof msg));
    CHECK(invalid_ids(nullptr, 1, 100, msg, sizeof msg) && std::strstr(msg, "null id list"));
    CHECK(invalid_ids(good, -1, 100, msg, sizeof msg) && std::strstr(msg, "-1"));
    const int64_t neg[] = {3, -7}, big[] = {100};
    CHECK(invalid_ids(neg, 2, 100, msg, sizeof msg) && std::strstr(msg, "id -7"));
    CHECK(invalid_ids(big, 1, 100, msg, sizeof msg) && std::strstr(msg, "id 100"));
    // set / test / count, with a base: ids outside [base, base + n) match nothing, duplicates count once
    for (int64_t n : {0, 1, 7, 8, 9, 31, 32, 33, 64, 65, 257}) {
        Bitmap b;
        b.reset(1000, n);
        CHECK(b.w.size() == (words_for(n) ? words_for(n) : 1) && b.count == 0);
        std::vector<int64_t> ids;
        for (int64_t i = 0; i < n; i += 3) ids.push_back(1000 + i), ids.push_back(1000 + i);
        ids.push_back(999);
        ids.push_back(1000 + n);
        b.add(ids.data(), static_cast<int64_t>(ids.size()));
        CHECK(b.count == (n + 2) / 3);
        CHECK(popcount(b.w.data(), n) == b.count);
        for (int64_t i = -2; i < n + 40; ++i) CHECK(b.test(i) == (i >= 0 && i < n && i % 3 == 0));
        b.add(ids.data(), static_cast<int64_t>(ids.size()));
        CHECK(b.count == (n + 2) / 3);
        mi355rec_rowset s;
        s.bits = b;
        for (int64_t i = 0; i < n; ++i) {
            CHECK(admits(&s, true, i) == (i % 3 == 0));
            CHECK(admits(&s, false, i) == (i % 3 != 0));
            CHECK(admits(nullptr, true, i) && admits(nullptr, false, i));
        }
    }
    // slices: every lo and hi of a 200-bit pattern against a bit-by-bit loop; the padding bits are 0
    const int64_t n = 200;
    Bitmap b;
    b.reset(0, n);
    uint32_t x = 12345u;
    for (int64_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        if (x >> 31) b.add(&i, 1);
    }
    for (int64_t lo = 0; lo <= n; ++lo)
        for (int64_t hi = lo; hi <= n; ++hi) {
            std::vector<uint32_t> dst(words_for(hi - lo) + 1, 0xffffffffu);   // one guard word behind
            slice(b.w.data(), lo, hi, dst.data());
            CHECK(dst.back() == 0xffffffffu);
            int64_t c = 0;
            for (int64_t i = 0; i < static_cast<int64_t>(words_for(hi - lo)) * 32; ++i) {
                const bool want = i < hi - lo && b.test(lo + i);
                CHECK(test_bit(dst.data(), i) == want);
                c += want;
            }
            CHECK(popcount(dst.data(), hi - lo) == c);
        }
    return 0;
}

static int slice_file(const char* in_path, const char* out_path) {
    using namespace mi355rowset;
    std::FILE* in = std::fopen(in_path, "rb");
    CHECK(in);
    int64_t head[2];
    CHECK(std::fread(head, sizeof head, 1, in) == 1);
    std::vector<uint32_t> words(words_for(head[0]) ? words_for(head[0]) : 1);
    CHECK(std::fread(words.data(), sizeof(uint32_t), words_for(head[0]), in) == words_for(head[0]));
    std::vector<int64_t> pairs(static_cast<size_t>(2 * head[1]));
    CHECK(std::fread(pairs.data(), sizeof(int64_t), pairs.size(), in) == pairs.size());
    std::fclose(in);
    std::FILE* out = std::fopen(out_path, "wb");
    CHECK(out);
    for (int64_t p = 0; p < head[1]; ++p) {
        const int64_t lo = pairs[static_cast<size_t>(2 * p)], hi = pairs[static_cast<size_t>(2 * p + 1)];
        std::vector<uint32_t> dst(words_for(hi - lo) ? words_for(hi - lo) : 1, 0u);
        slice(words.data(), lo, hi, dst.data());
        const int64_t c = popcount(dst.data(), hi - lo);
        CHECK(std::fwrite(dst.data(), sizeof(uint32_t), words_for(hi - lo), out) == words_for(hi - lo));
        CHECK(std::fwrite(&c, sizeof c, 1, out) == 1);
    }
    CHECK(std::fclose(out) == 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "slice") return slice_file(argv[2], argv[3]);
    if (argc != 1) {
        std::fprintf(stderr, "usage: rowset_check [slice IN OUT]\n");
        return 2;
    }
    const int rc = self_checks();
    if (rc == 0) std::printf("rowset.h: ok\n");
    return rc;
}
