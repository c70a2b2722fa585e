// The host side of BOUNDED REQUESTS (csrc/playlist_request.h: from_request for mi355rec_bounded_query_t, bounded_floor,
// bounded_radius_floor, bounded_match, bounded_cut) in a stand-alone program, for AddressSanitizer and UBSan: every valid size of the
// struct read from a buffer of exactly that many bytes (read_sized must not look past it), every refusal, the floor's properties.
// Built and run by tests/test_bounded_cpu.py as its own process.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "playlist_request.h"

using namespace mi355playlist;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

// The conversion of the first `size` bytes of `q`, from a heap buffer of exactly that size.
static bool convert(const mi355rec_bounded_query_t& q, uint32_t size, const mi355rec_request_ext_t* ext, const mi355rec_bounded_result_t& res,
                    Request* r, Outputs* out, char* msg, size_t cap) {
    std::vector<unsigned char> exact(size ? size : 1);
    mi355rec_bounded_query_t head = q;
    head.size = size;
    std::memcpy(exact.data(), &head, size < sizeof head ? size : sizeof head);
    mi355rec_bounded_query_t full;
    // (a struct shorter than its size field cannot say its size: those sizes are refused before anything is read)
    if (size < sizeof(uint32_t)) {
        mi355rec_bounded_query_t tiny = head;
        return from_request(&tiny, ext, &res, &full, r, out, msg, cap);
    }
    return from_request(reinterpret_cast<const mi355rec_bounded_query_t*>(exact.data()), ext, &res, &full, r, out, msg, cap);
}

int main() {
    char msg[160];
    float members[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    int64_t rows[2] = {3, 4}, idx[8], total = -1;
    float score[8];
    int count = -1;
    const mi355rec_bounded_result_t res = {idx, score, &count, &total};
    mi355rec_bounded_query_t q;
    std::memset(&q, 0, sizeof q);
    q.members = members;
    q.k = 1;
    q.topn = 8;
    q.metric = MI355REC_BOUNDED_COSINE;
    q.bound = 0.5f;
    Request r;
    Outputs out;

    // every size: the ends of the fields convert (or are refused for what they leave zero), everything else is refused by its size
    const uint32_t ends[] = {4, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72};
    for (uint32_t size = 0; size <= 80; ++size) {
        bool is_end = false;
        for (uint32_t e : ends) is_end = is_end || e == size;
        const bool refused = convert(q, size, nullptr, res, &r, &out, msg, sizeof msg);
        if (!is_end) CHECK(refused && std::strstr(msg, "not the end of a field of the 72 bytes") != nullptr);
        else if (size < 16) CHECK(refused && std::strstr(msg, "needs members") != nullptr);
        else {
            CHECK(!refused);
            CHECK(r.bounded && r.k == (size >= 52 ? 1 : 0) && r.topn == (size >= 64 ? 8 : 0));
            CHECK(r.floor_score == (size >= 72 ? 0.5f : 0.0f) && r.floor_thr == bounded_floor(r.floor_score));
            CHECK(out.total == &total && out.idx == idx && out.member == nullptr);
        }
    }
    // the refusals of the struct's own fields
    struct Bad { float bound; int metric; uint32_t flags; const char* text; };
    const Bad bad[] = {{std::numeric_limits<float>::quiet_NaN(), 0, 0, "a floor is finite"}, {std::numeric_limits<float>::infinity(), 1, 0, "a radius is finite"},
                       {-1.0f, 1, 0, "a radius is >= 0"}, {0.5f, 2, 0, "MI355REC_BOUNDED_COSINE (0) or"}, {0.5f, 0, 4, "must be 0"}};
    for (const Bad& b : bad) {
        mi355rec_bounded_query_t x = q;
        x.bound = b.bound, x.metric = b.metric, x.flags = b.flags;
        CHECK(convert(x, sizeof x, nullptr, res, &r, &out, msg, sizeof msg) && std::strstr(msg, b.text) != nullptr);
    }
    {
        mi355rec_bounded_query_t x = q;
        x.rows = rows;
        CHECK(convert(x, sizeof x, nullptr, res, &r, &out, msg, sizeof msg) && std::strstr(msg, "by value and by row") != nullptr);
        mi355rec_bounded_result_t none = res;
        none.out_total = nullptr;
        CHECK(convert(q, sizeof q, nullptr, none, &r, &out, msg, sizeof msg) && std::strstr(msg, "null out_total") != nullptr);
        none = res;
        none.out_idx = nullptr;
        CHECK(convert(q, sizeof q, nullptr, none, &r, &out, msg, sizeof msg) && std::strstr(msg, "null out_idx") != nullptr);
        x = q;
        x.topn = 0;
        CHECK(!convert(x, sizeof x, nullptr, none, &r, &out, msg, sizeof msg) && out.idx == nullptr && r.topn == 0);
        float scales[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
        mi355rec_request_ext_t ext = scales_only_ext(scales);
        CHECK(convert(q, sizeof q, &ext, res, &r, &out, msg, sizeof msg) && std::strcmp(msg, "bounded requests take no feature scales") == 0);
        CHECK(from_request(static_cast<const mi355rec_bounded_query_t*>(nullptr), nullptr, &res, &x, &r, &out, msg, sizeof msg));
    }
    // the floor: a key matches iff its score's image is at least b's; -0.0 and +0.0 are one
    CHECK(bounded_floor(0.0f) == bounded_floor(-0.0f) && bounded_match(-0.0f, 0.0f) && bounded_match(0.0f, -0.0f));
    CHECK(bounded_match(0.5f, 0.5f) && !bounded_match(std::nextafter(0.5f, 0.0f), 0.5f) && bounded_match(-0.25f, -0.5f) && !bounded_match(-0.75f, -0.5f));
    CHECK(bounded_floor(0.5f) + 1 == (static_cast<uint64_t>(ordered_image(0.5f)) << 32));
    // the radius: m_max is the largest float whose root is <= the radius
    const float top = std::numeric_limits<float>::max();
    const float radii[] = {0.0f, 1e-30f, 1e-20f, 0.1f, 0.3f, 1.0f, 1.5f, 3.0f, 1e10f, 1.8e19f, 1.9e19f, 1e30f, top, std::nextafter(1.0f, 2.0f),
                           std::nextafter(1.0f, 0.0f), 1.4142135f, 1e-22f, std::numeric_limits<float>::denorm_min()};
    for (float radius : radii) {
        const float m = 0.0f - bounded_radius_floor(radius);
        CHECK(m >= 0.0f && m <= top && std::sqrt(m) <= radius);
        CHECK(m == top || std::sqrt(std::nextafter(m, top)) > radius);
    }
    // the host's cut of a merged list
    {
        Request b;
        b.bounded = true;
        b.floor_score = 0.5f;
        const int64_t ids[5] = {9, 8, 7, -1, -1};
        const float sc[5] = {0.9f, 0.5f, 0.4999f, 0.0f, 0.0f};
        CHECK(bounded_cut(b, ids, sc, 5) == 2 && bounded_cut(b, ids, sc, 1) == 1 && bounded_cut(b, ids, sc, 0) == 0);
        b.floor_score = -1.0f;
        CHECK(bounded_cut(b, ids, sc, 5) == 3);
    }
    if (failures) return 1;
    std::printf("bounded requests (playlist_request.h): ok\n");
    return 0;
}
