// embed_multi_check.cpp — csrc/embed_multi_request.h as a stand-alone program (its own main), built by
// tests/test_embed_multi_cpu.py with -fsanitize=address,undefined: the request and the result read from heap buffers of
// exactly their size, every refusal with its text, the plain statement of THE VALUE (V = the largest finite v_k, the
// interest = the lowest k that gives it: the all-non-finite row, the -0.0 / +0.0 tie, equal values at two interests) and THE
// MERGE of identity 2 (K single-interest top-N lists against the top-N by V) on small random tables.  No pointer named
// *_dev is dereferenced by the header: the ones given here are small integers on purpose.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "embed_multi_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using namespace mi355embedmulti;

const float* fake_floats = reinterpret_cast<const float*>(uintptr_t{0x1000});     // "device" pointers: aligned, never read
const int64_t* fake_ids = reinterpret_cast<const int64_t*>(uintptr_t{0x2000});
int64_t* fake_idx = reinterpret_cast<int64_t*>(uintptr_t{0x3000});

bool has(const char* msg, const char* text) { return std::strstr(msg, text) != nullptr; }

mi355rec_embed_multi_result_t good_result() {
    mi355rec_embed_multi_result_t res{};
    res.size = sizeof res;
    res.out_idx_dev = fake_idx;
    return res;
}

mi355rec_embed_multi_query_t good_query() {
    mi355rec_embed_multi_query_t q{};
    q.size = sizeof q;
    q.interests_dev = fake_floats;
    q.n_interests = 5;
    q.audio_row = -1;
    q.topn = 10;
    q.metric = MI355REC_EMBED_COSINE;
    q.w_embed = 1.0f;
    return q;
}

// The request and the result from heap copies of exactly their `size` bytes, as a caller with an older header hands them over.
template <class T>
std::unique_ptr<char[]> heap_copy(const T& x) {
    const size_t n = std::max<size_t>(x.size, sizeof x.size);   // (`size` itself is always there)
    std::unique_ptr<char[]> b(new char[n]);
    std::memcpy(b.get(), &x, std::min(n, sizeof x));
    return b;
}

bool refuse(const mi355rec_embed_multi_query_t& q, const mi355rec_embed_multi_result_t& res, char* msg, size_t cap, Query* out = nullptr,
            int64_t n_rows = 100) {
    const auto qb = heap_copy(q), rb = heap_copy(res);
    mi355rec_embed_multi_query_t full;
    mi355rec_embed_multi_result_t fres;
    Query r;
    msg[0] = 0;
    const bool refused = from_multi_query(reinterpret_cast<const mi355rec_embed_multi_query_t*>(qb.get()),
                                          reinterpret_cast<const mi355rec_embed_multi_result_t*>(rb.get()), n_rows, &full, &fres, &r, msg, cap);
    if (out) *out = r;
    return refused;
}

void check_layout() {
    using Q = mi355rec_embed_multi_query_t;
    using R = mi355rec_embed_multi_result_t;
    using I = mi355rec_embed_multi_info_t;
    EXPECT(sizeof(Q) == 72 && offsetof(Q, interests_dev) == 8 && offsetof(Q, audio) == 16 && offsetof(Q, exclude_dev) == 24 && offsetof(Q, audio_row) == 32);
    EXPECT(offsetof(Q, n_interests) == 40 && offsetof(Q, n_exclude) == 44 && offsetof(Q, topn) == 48 && offsetof(Q, metric) == 52);
    EXPECT(offsetof(Q, w_audio) == 56 && offsetof(Q, w_embed) == 60 && offsetof(Q, reserved) == 64);
    EXPECT(sizeof(R) == 40 && offsetof(R, out_idx_dev) == 8 && offsetof(R, out_score_dev) == 16 && offsetof(R, out_count_dev) == 24 &&
           offsetof(R, out_interest_dev) == 32);
    EXPECT(offsetof(R, out_count_dev) == offsetof(mi355rec_embed_stream_result_t, out_count_dev) && sizeof(mi355rec_embed_stream_result_t) == 32);
    EXPECT(sizeof(I) == 96 && offsetof(I, table_dev) == 40 && offsetof(I, borrowed) == 76 && offsetof(I, max_interests) == 80);
    EXPECT(offsetof(I, pass_interests) == 84 && offsetof(I, query_launches) == 88 && offsetof(I, reserved) == 92);
    EXPECT(offsetof(I, pass_users) == offsetof(mi355rec_embed_stream_info_t, pass_users) && offsetof(I, launches) == offsetof(mi355rec_embed_stream_info_t, launches));
    EXPECT(MI355REC_EMBED_MULTI_MAX_INTERESTS == 32 && MI355REC_EMBED_MULTI_MAX_EXCLUDE == MI355REC_EMBED_STREAM_MAX_EXCLUDE);
}

void check_refusals() {
    char msg[256];
    Query r;
    // a handle on the CPU placement (mi355rec_stats reports device -1 there) carries no table
    msg[0] = 0;
    EXPECT(invalid_handle(-1, msg, sizeof msg) && has(msg, "need a handle on a HIP device (the CPU placement is not served)"));
    msg[0] = 0;
    EXPECT(!invalid_handle(0, msg, sizeof msg) && !invalid_handle(7, msg, sizeof msg) && msg[0] == 0);
    EXPECT(!refuse(good_query(), good_result(), msg, sizeof msg, &r));
    EXPECT(r.interests_dev == fake_floats && r.n_interests == 5 && r.topn == 10 && r.n_exclude == 0 && !r.use_audio && r.w_embed == 1.0f);
    {
        mi355rec_embed_multi_query_t full;
        mi355rec_embed_multi_result_t fres;
        const auto q = good_query();
        const auto res = good_result();
        EXPECT(from_multi_query(nullptr, &res, 100, &full, &fres, &r, msg, sizeof msg) && has(msg, "null argument"));
        EXPECT(from_multi_query(&q, nullptr, 100, &full, &fres, &r, msg, sizeof msg) && has(msg, "null argument"));
    }
    // sizes: the end of every field is served; anything else, 0 and more than the struct are refused
    const size_t ends[] = {4, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 72};
    for (uint32_t size = 0; size <= 80; ++size) {
        auto q = good_query();
        q.size = size;
        const bool known = std::find(std::begin(ends), std::end(ends), size) != std::end(ends);
        const bool refused = refuse(q, good_result(), msg, sizeof msg);
        if (!known) EXPECT(refused && has(msg, "embed multi query of size") && has(msg, "not the end of a field of the 72 bytes"));
        else if (size < 44) EXPECT(refused && has(msg, "n_interests 0 out of [1, 32]"));   // (a struct that ends before n_interests reads it as zero)
        else if (size < 64) EXPECT(refused && has(msg, "embed_weight 0"));
        else EXPECT(!refused);
    }
    const size_t rends[] = {4, 8, 16, 24, 32, 40};
    for (uint32_t size = 0; size <= 48; ++size) {
        auto res = good_result();
        res.size = size;
        const bool known = std::find(std::begin(rends), std::end(rends), size) != std::end(rends);
        const bool refused = refuse(good_query(), res, msg, sizeof msg);
        if (!known) EXPECT(refused && has(msg, "embed multi result of size") && has(msg, "40 bytes"));
        else if (size < 16) EXPECT(refused && has(msg, "null out_idx_dev"));
        else EXPECT(!refused);   // (scores, the count and the interests are optional)
    }
    auto res = good_result();
    res.out_idx_dev = nullptr;
    EXPECT(refuse(good_query(), res, msg, sizeof msg) && has(msg, "null out_idx_dev in an embed multi result"));
    res = good_result();
    res.reserved = 1;
    EXPECT(refuse(good_query(), res, msg, sizeof msg) && has(msg, "reserved 0x1 in an embed multi result: must be 0"));

    auto q = good_query();
    q.flags = 2;
    EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "flags 0x2") && has(msg, "must be 0"));
    q = good_query();
    q.reserved = 7;
    EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "reserved 0x7"));
    q = good_query();
    q.reserved = uint64_t{1} << 40;   // (the high half is read too)
    EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "reserved 0x10000000000"));
    for (int K : {0, -1, 33, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        q = good_query();
        q.n_interests = K;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "n_interests") && has(msg, "out of [1, 32]"));
    }
    for (int K : {1, 32}) {
        q = good_query();
        q.n_interests = K;
        EXPECT(!refuse(q, good_result(), msg, sizeof msg, &r) && r.n_interests == K);
    }
    q = good_query();
    q.interests_dev = nullptr;
    EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "null interests_dev") && has(msg, "interests by rows are not served"));
    for (uintptr_t off : {uintptr_t{4}, uintptr_t{8}, uintptr_t{1}}) {
        q = good_query();
        q.interests_dev = reinterpret_cast<const float*>(uintptr_t{0x1000} + off);
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "interests_dev is not 16-byte aligned"));
    }
    for (int metric : {-1, 2}) {
        q = good_query();
        q.metric = metric;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "MI355REC_EMBED_COSINE (0) or MI355REC_EMBED_DOT (1)"));
    }
    q = good_query();
    q.metric = MI355REC_EMBED_DOT;
    EXPECT(!refuse(q, good_result(), msg, sizeof msg, &r) && r.metric == MI355REC_EMBED_DOT);
    for (float w : {0.0f, -0.0f, 4.5f, -4.5f, NAN, INFINITY}) {
        q = good_query();
        q.w_embed = w;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "embed_weight") && has(msg, "finite, not 0 and at most 4"));
    }
    for (float w : {4.5f, NAN, -INFINITY}) {
        q = good_query();
        q.w_audio = w;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "audio_weight") && has(msg, "finite and at most 4"));
    }
    for (int64_t row : {int64_t{-1}, int64_t{100}, int64_t{1} << 40}) {   // w_audio != 0 needs a row of the handle, or audio by value
        q = good_query();
        q.w_audio = 1.0f;
        q.audio_row = row;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "needs audio by value or a valid audio_row"));
        float audio[12] = {};
        q.audio = audio;
        EXPECT(!refuse(q, good_result(), msg, sizeof msg, &r) && r.use_audio && r.audio == audio && r.audio_row == -1);
    }
    q = good_query();
    q.w_audio = -4.0f;
    q.audio_row = 99;
    EXPECT(!refuse(q, good_result(), msg, sizeof msg, &r) && r.use_audio && r.audio_row == 99 && r.audio == nullptr);
    for (int topn : {0, -3, 1025}) {
        q = good_query();
        q.topn = topn;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "topn") && has(msg, "out of [1, 1024]"));
    }
    for (int L : {-1, 1025}) {
        q = good_query();
        q.n_exclude = L;
        q.exclude_dev = fake_ids;
        EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "n_exclude") && has(msg, "out of [0, 1024]"));
    }
    q = good_query();
    q.n_exclude = 5;
    EXPECT(refuse(q, good_result(), msg, sizeof msg) && has(msg, "null exclusion list with n_exclude 5"));
    q.exclude_dev = fake_ids;
    q.n_exclude = 1024;
    EXPECT(!refuse(q, good_result(), msg, sizeof msg, &r) && r.n_exclude == 1024 && r.exclude_dev == fake_ids);
}

uint32_t bits_of(float x) {
    uint32_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

void check_value() {
    const float inf = INFINITY, nan = NAN;
    float V = 123.0f;
    int k = 77;
    {   // no finite value: no key, nothing written
        const float v[] = {nan, inf, -inf, nan};
        EXPECT(!multi_value(v, 4, &V, &k) && V == 123.0f && k == 77);
    }
    {   // a finite value among non-finite ones, however low: +inf is not a maximum
        const float v[] = {inf, nan, -3.0e38f, -inf};
        EXPECT(multi_value(v, 4, &V, &k) && V == -3.0e38f && k == 2);
    }
    {   // -0.0 before +0.0 and the reverse: equal, so the first holds, and the key reports +0.0 either way
        const float a[] = {-1.0f, -0.0f, 0.0f};
        EXPECT(multi_value(a, 3, &V, &k) && k == 1 && bits_of(V) == 0x80000000u);
        const uint64_t key_a = key_of(V, 9);
        const float b[] = {-1.0f, 0.0f, -0.0f};
        EXPECT(multi_value(b, 3, &V, &k) && k == 1 && bits_of(V) == 0u);
        EXPECT(key_of(V, 9) == key_a && (key_a >> 32) == 0x80000000u);
    }
    {   // equal values at two interests: the lower index
        const float v[] = {0.25f, 0.75f, 0.5f, 0.75f, nan};
        EXPECT(multi_value(v, 5, &V, &k) && V == 0.75f && k == 1);
        EXPECT(multi_value(v, 1, &V, &k) && V == 0.25f && k == 0);
    }
    // keys order by value, then by the lower row
    EXPECT(key_of(1.0f, 5) > key_of(0.5f, 1) && key_of(-0.5f, 5) > key_of(-1.0f, 1) && key_of(0.0f, 0) > key_of(-1e-30f, 0));
    EXPECT(key_of(0.5f, 3) > key_of(0.5f, 4) && key_of(-3.0e38f, 0xFFFFFFFEu) != 0);
}

// Identity 2 on a table of n rows and K interests whose v_k are drawn from a few values (ties everywhere), with
// non-finite entries: the merge of the K top-N lists is the top-N by V, with its interests.
void check_merge_once(std::mt19937& rng, int n, int K, int topn, uint32_t row_base) {
    const float pool[] = {-2.0f, -1.0f, -0.0f, 0.0f, 0.5f, 0.5f, 1.0f, 3.0e38f, -3.0e38f, NAN, INFINITY, -INFINITY, 1e-40f};
    std::vector<float> v(static_cast<size_t>(K) * n);
    for (auto& x : v) {
        const uint32_t pick = rng() % 20;
        x = pick < 13 ? pool[pick] : static_cast<float>(static_cast<int>(rng() % 2001) - 1000) / 1000.0f;
    }
    // the statement: V and the interest per row, keys in order
    struct Entry {
        uint64_t key;
        int interest;
    };
    std::vector<Entry> direct;
    for (int row = 0; row < n; ++row) {
        std::vector<float> mine(static_cast<size_t>(K));
        for (int k = 0; k < K; ++k) mine[static_cast<size_t>(k)] = v[static_cast<size_t>(k) * n + row];
        float V;
        int who;
        if (multi_value(mine.data(), K, &V, &who)) direct.push_back({key_of(V, row_base + static_cast<uint32_t>(row)), who});
    }
    std::sort(direct.begin(), direct.end(), [](const Entry& a, const Entry& b) { return a.key > b.key; });
    if (static_cast<int>(direct.size()) > topn) direct.resize(static_cast<size_t>(topn));
    // the K single-interest answers: heap blocks of exactly K * topn keys
    std::unique_ptr<uint64_t[]> keys(new uint64_t[static_cast<size_t>(K) * topn]);
    std::unique_ptr<int[]> counts(new int[K]);
    for (int k = 0; k < K; ++k) {
        std::vector<uint64_t> mine;
        for (int row = 0; row < n; ++row) {
            const float x = v[static_cast<size_t>(k) * n + row];
            if (std::isfinite(x)) mine.push_back(key_of(x, row_base + static_cast<uint32_t>(row)));
        }
        std::sort(mine.begin(), mine.end(), std::greater<uint64_t>());
        counts[k] = static_cast<int>(std::min<size_t>(mine.size(), static_cast<size_t>(topn)));
        for (int i = 0; i < topn; ++i) keys[static_cast<size_t>(k) * topn + i] = i < counts[k] ? mine[static_cast<size_t>(i)] : 0ull;
    }
    std::unique_ptr<uint64_t[]> out_keys(new uint64_t[topn]);
    std::unique_ptr<int32_t[]> out_interest(new int32_t[topn]);
    const int got = merge_lists(keys.get(), counts.get(), K, topn, out_keys.get(), out_interest.get());
    EXPECT(got == static_cast<int>(direct.size()));
    for (int i = 0; i < got && i < static_cast<int>(direct.size()); ++i) {
        EXPECT(out_keys[i] == direct[static_cast<size_t>(i)].key);
        EXPECT(out_interest[i] == direct[static_cast<size_t>(i)].interest);
    }
}

void check_merge() {
    std::mt19937 rng(11);
    for (int n : {1, 2, 17, 100, 257})
        for (int K : {1, 2, 3, 5, 32})
            for (int topn : {1, 10, 64, 300})
                check_merge_once(rng, n, K, topn, n == 17 ? 4000000000u : 0u);
}

}  // namespace

int main() {
    check_layout();
    check_refusals();
    check_value();
    check_merge();
    if (failures) {
        std::printf("embed_multi_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_multi_request.h: ok\n");
    return 0;
}
