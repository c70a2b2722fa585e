// embed_half_check.cpp — csrc/embed_half_request.h as a stand-alone program (its own main), built by
// tests/test_embed_half_cpu.py with -fsanitize=address,undefined: W(x) of all 65 536 words of both storages against a
// table-free restatement (the value assembled from sign, exponent and significand with ldexp), the create checks of a half
// table, and a request read through embed_request.h's from_query from a buffer of exactly its size, as the library reads it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "embed_half_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

void check_widening() {
    using namespace mi355embedhalf;
    int nans = 0, subnormals = 0;
    for (uint32_t w = 0; w < 65536u; ++w) {
        const uint16_t word = static_cast<uint16_t>(w);
        // fp16: (-1)^s * 2^(e-15) * (1 + m/1024), subnormal: (-1)^s * 2^-14 * (m/1024); every such value is an fp32
        const int s = w >> 15, e = (w >> 10) & 31, m = w & 1023;
        const float got = widen(word, MI355REC_EMBED_HALF_FP16);
        if (e == 31 && m != 0) {
            EXPECT(std::isnan(got) && std::signbit(got) == (s != 0));
            ++nans;
        } else {
            float want = e == 31 ? INFINITY : e == 0 ? std::ldexp(static_cast<float>(m), -24) : std::ldexp(static_cast<float>(1024 + m), e - 25);
            if (s) want = -want;
            EXPECT(bits_of(got) == bits_of(want));
            if (e == 0 && m != 0) {
                EXPECT(got != 0.0f && std::fpclassify(got) == FP_NORMAL);   // exact, never flushed
                ++subnormals;
            }
        }
        // bf16: the fp32 whose upper half the word is
        const float b = widen(word, MI355REC_EMBED_HALF_BF16);
        EXPECT((bits_of(b) >> 16) == w && (bits_of(b) & 0xffffu) == 0u);
        const int be = (w >> 7) & 255, bm = w & 127;
        if (be == 255 && bm != 0) {
            EXPECT(std::isnan(b));
        } else {
            float want = be == 255 ? INFINITY : be == 0 ? std::ldexp(static_cast<float>(bm), -133) : std::ldexp(static_cast<float>(128 + bm), be - 134);
            if (s) want = -want;
            EXPECT(bits_of(b) == bits_of(want));
        }
    }
    EXPECT(nans == 2 * 1023 && subnormals == 2 * 1023);
    EXPECT(widen(0x7bffu, MI355REC_EMBED_HALF_FP16) == 65504.0f && widen(0x0001u, MI355REC_EMBED_HALF_FP16) == std::ldexp(1.0f, -24));
    EXPECT(std::isinf(widen(0x7c00u, MI355REC_EMBED_HALF_FP16)) && bits_of(widen(0x8000u, MI355REC_EMBED_HALF_FP16)) == 0x80000000u);
}

void check_create() {
    using namespace mi355embedhalf;
    char msg[256];
    std::unique_ptr<uint16_t[]> words(new uint16_t[4 * 16]());
    for (int storage : {MI355REC_EMBED_HALF_FP16, MI355REC_EMBED_HALF_BF16}) {
        for (int dim : {16, 32, 64, 128}) EXPECT(!invalid_table(words.get(), 4, dim, storage, 4, msg, sizeof msg));
        for (int dim : {0, 8, 12, 24, 256, -16}) EXPECT(invalid_table(words.get(), 4, dim, storage, 4, msg, sizeof msg) && std::strstr(msg, "embedding dim"));
        EXPECT(invalid_table(words.get(), 4, 16, storage, 5, msg, sizeof msg) && std::strstr(msg, "table of 4 rows for a handle of 5 rows"));
        EXPECT(invalid_table(nullptr, 4, 16, storage, 4, msg, sizeof msg) && std::strstr(msg, "null table"));
        EXPECT(!invalid_table(nullptr, 0, 16, storage, 0, msg, sizeof msg));
    }
    for (int storage : {-1, 2, 16}) EXPECT(invalid_table(words.get(), 4, 16, storage, 4, msg, sizeof msg) && std::strstr(msg, "storage"));
    char tiny[8];
    EXPECT(invalid_table(words.get(), 4, 16, 7, 4, tiny, sizeof tiny) && tiny[7] == 0);   // a message longer than its buffer
}

// The half library reads its requests with embed_request.h's from_query: the struct from a heap buffer of exactly its size.
void check_request() {
    using namespace mi355embed;
    std::vector<int64_t> rows = {3, 1, 2}, idx(8);
    mi355rec_embed_query_t q{};
    q.size = sizeof q;
    q.rows = rows.data();
    q.k = 3;
    q.topn = 8;
    q.w_embed = 0.5f;
    std::unique_ptr<unsigned char[]> buf(new unsigned char[sizeof q]);
    std::memcpy(buf.get(), &q, sizeof q);
    mi355rec_embed_result_t res{};
    res.size = sizeof res;
    res.out_idx = idx.data();
    mi355rec_embed_query_t full;
    mi355rec_embed_result_t fres;
    Request r;
    char msg[256];
    EXPECT(!from_query(reinterpret_cast<const mi355rec_embed_query_t*>(buf.get()), &res, true, 4, &full, &fres, &r, msg, sizeof msg));
    EXPECT(r.k == 3 && r.rows == rows.data() && !r.use_audio && r.topn == 8);
    EXPECT(from_query(reinterpret_cast<const mi355rec_embed_query_t*>(buf.get()), &res, true, 3, &full, &fres, &r, msg, sizeof msg) &&
           std::strstr(msg, "Invalid song index: 3"));
}

}  // namespace

int main() {
    check_widening();
    check_create();
    check_request();
    if (failures) {
        std::printf("embed_half_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_half_request.h: ok\n");
    return 0;
}
