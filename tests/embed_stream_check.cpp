// embed_stream_check.cpp — csrc/embed_stream_request.h as a stand-alone program (its own main), built by
// tests/test_embed_stream_cpu.py with -fsanitize=address,undefined: the two requests and the result read from heap buffers of
// exactly their size, every refusal with its text, the create checks, the PREPARE statement (map, sentinel, bitonic sort)
// against std::sort + std::unique membership on hostile lists, and the FINISH statement against mi355embed::write_result.
// No pointer named *_dev is dereferenced by the header: the ones given here are small integers on purpose.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "embed_stream_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using namespace mi355embedstream;

const float* fake_floats = reinterpret_cast<const float*>(uintptr_t{0x1000});     // "device" pointers: aligned, never read
const int64_t* fake_ids = reinterpret_cast<const int64_t*>(uintptr_t{0x2000});
int64_t* fake_idx = reinterpret_cast<int64_t*>(uintptr_t{0x3000});

bool has(const char* msg, const char* text) { return std::strstr(msg, text) != nullptr; }

mi355rec_embed_stream_result_t good_result() {
    mi355rec_embed_stream_result_t res{};
    res.size = sizeof res;
    res.out_idx_dev = fake_idx;
    return res;
}

mi355rec_embed_stream_query_t good_query() {
    mi355rec_embed_stream_query_t q{};
    q.size = sizeof q;
    q.user_dev = fake_floats;
    q.audio_row = -1;
    q.topn = 10;
    q.metric = MI355REC_EMBED_COSINE;
    q.w_embed = 1.0f;
    return q;
}

mi355rec_embed_stream_users_t good_users() {
    mi355rec_embed_stream_users_t q{};
    q.size = sizeof q;
    q.users_dev = fake_floats;
    q.n_users = 3;
    q.topn = 10;
    q.metric = MI355REC_EMBED_DOT;
    q.w_embed = -0.5f;
    return q;
}

// The request from a heap copy of exactly q.size bytes, as a caller with an older header hands it over.
bool refuse_query(const mi355rec_embed_stream_query_t& q, const mi355rec_embed_stream_result_t& res, char* msg, size_t cap, Query* out = nullptr,
                  int64_t n_rows = 100) {
    const size_t qn = std::max<size_t>(q.size, sizeof q.size), rn = std::max<size_t>(res.size, sizeof res.size);   // (`size` itself is always there)
    std::unique_ptr<char[]> qb(new char[qn]), rb(new char[rn]);
    std::memcpy(qb.get(), &q, std::min(qn, sizeof q));
    std::memcpy(rb.get(), &res, std::min(rn, sizeof res));
    mi355rec_embed_stream_query_t full;
    mi355rec_embed_stream_result_t fres;
    Query r;
    msg[0] = 0;
    const bool refused = from_stream_query(reinterpret_cast<const mi355rec_embed_stream_query_t*>(qb.get()),
                                           reinterpret_cast<const mi355rec_embed_stream_result_t*>(rb.get()), n_rows, &full, &fres, &r, msg, cap);
    if (out) *out = r;
    return refused;
}

bool refuse_users(const mi355rec_embed_stream_users_t& q, const mi355rec_embed_stream_result_t& res, char* msg, size_t cap, Users* out = nullptr) {
    const size_t qn = std::max<size_t>(q.size, sizeof q.size), rn = std::max<size_t>(res.size, sizeof res.size);   // (`size` itself is always there)
    std::unique_ptr<char[]> qb(new char[qn]), rb(new char[rn]);
    std::memcpy(qb.get(), &q, std::min(qn, sizeof q));
    std::memcpy(rb.get(), &res, std::min(rn, sizeof res));
    mi355rec_embed_stream_users_t full;
    mi355rec_embed_stream_result_t fres;
    Users r;
    msg[0] = 0;
    const bool refused = from_stream_users(reinterpret_cast<const mi355rec_embed_stream_users_t*>(qb.get()),
                                           reinterpret_cast<const mi355rec_embed_stream_result_t*>(rb.get()), &full, &fres, &r, msg, cap);
    if (out) *out = r;
    return refused;
}

void check_layout() {
    using Q = mi355rec_embed_stream_query_t;
    using U = mi355rec_embed_stream_users_t;
    using R = mi355rec_embed_stream_result_t;
    using I = mi355rec_embed_stream_info_t;
    EXPECT(sizeof(Q) == 64 && offsetof(Q, user_dev) == 8 && offsetof(Q, audio) == 16 && offsetof(Q, exclude_dev) == 24 && offsetof(Q, audio_row) == 32);
    EXPECT(offsetof(Q, n_exclude) == 40 && offsetof(Q, topn) == 44 && offsetof(Q, metric) == 48 && offsetof(Q, w_audio) == 52 && offsetof(Q, w_embed) == 56);
    EXPECT(sizeof(U) == 48 && offsetof(U, users_dev) == 8 && offsetof(U, exclude_dev) == 16 && offsetof(U, n_users) == 24 && offsetof(U, topn) == 28);
    EXPECT(offsetof(U, exclude_len) == 32 && offsetof(U, metric) == 36 && offsetof(U, w_embed) == 40 && offsetof(U, reserved) == 44);
    EXPECT(sizeof(R) == 32 && offsetof(R, out_idx_dev) == 8 && offsetof(R, out_score_dev) == 16 && offsetof(R, out_count_dev) == 24);
    EXPECT(sizeof(I) == 80 && offsetof(I, table_dev) == 40 && offsetof(I, launches) == 48 && offsetof(I, pass_users) == 72 && offsetof(I, borrowed) == 76);
}

void check_query_refusals() {
    char msg[256];
    Query r;
    EXPECT(!refuse_query(good_query(), good_result(), msg, sizeof msg, &r));
    EXPECT(r.user_dev == fake_floats && r.topn == 10 && r.n_exclude == 0 && !r.use_audio && r.w_embed == 1.0f && r.audio_row == -1);
    {
        mi355rec_embed_stream_query_t full;
        mi355rec_embed_stream_result_t fres;
        const auto q = good_query();
        const auto res = good_result();
        EXPECT(from_stream_query(nullptr, &res, 100, &full, &fres, &r, msg, sizeof msg) && has(msg, "null argument"));
        EXPECT(from_stream_query(&q, nullptr, 100, &full, &fres, &r, msg, sizeof msg) && has(msg, "null argument"));
    }
    // sizes: the end of every field is served; anything else, 0 and more than the struct are refused
    const size_t ends[] = {8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64};
    for (uint32_t size = 0; size <= 72; ++size) {
        auto q = good_query();
        q.size = size;
        const bool known = std::find(std::begin(ends), std::end(ends), size) != std::end(ends) || size == 4;
        const bool refused = refuse_query(q, good_result(), msg, sizeof msg);
        if (!known) {
            EXPECT(refused && has(msg, "embed stream query of size") && has(msg, "not the end of a field of the 64 bytes"));
        } else if (size < 16) {
            EXPECT(refused && has(msg, "null user_dev"));   // (a struct that ends before user_dev reads it as zero)
        } else if (size < 60) {
            EXPECT(refused);   // (topn, then w_embed read as zero)
        } else {
            EXPECT(!refused);
        }
    }
    for (uint32_t size : {0u, 4u, 7u, 12u, 20u, 28u, 31u, 33u, 40u}) {
        auto res = good_result();
        res.size = size;
        EXPECT(refuse_query(good_query(), res, msg, sizeof msg));
        if (size != 4u) EXPECT(has(msg, "embed stream result of size") && has(msg, "32 bytes"));
        else EXPECT(has(msg, "null out_idx_dev"));
    }
    for (uint32_t size : {8u, 16u, 24u}) {   // out_idx_dev ends at 16: shorter reads it as null, from there on score and count are optional
        auto res = good_result();
        res.size = size;
        EXPECT(refuse_query(good_query(), res, msg, sizeof msg) == (size < 16u));
    }
    auto res = good_result();
    res.out_idx_dev = nullptr;
    EXPECT(refuse_query(good_query(), res, msg, sizeof msg) && has(msg, "null out_idx_dev in an embed stream result"));
    res = good_result();
    res.reserved = 1;
    EXPECT(refuse_query(good_query(), res, msg, sizeof msg) && has(msg, "reserved 0x1 in an embed stream result: must be 0"));

    auto q = good_query();
    q.flags = 2;
    EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "flags 0x2") && has(msg, "must be 0"));
    q = good_query();
    q.reserved = 7;
    EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "reserved 0x7"));
    q = good_query();
    q.user_dev = nullptr;
    EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "null user_dev") && has(msg, "members by rows are not served"));
    q = good_query();
    q.user_dev = reinterpret_cast<const float*>(uintptr_t{0x1004});
    EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "user_dev is not 16-byte aligned"));
    for (int metric : {-1, 2}) {
        q = good_query();
        q.metric = metric;
        EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "MI355REC_EMBED_COSINE (0) or MI355REC_EMBED_DOT (1)"));
    }
    for (float w : {0.0f, -0.0f, 4.5f, -4.5f, NAN, INFINITY}) {
        q = good_query();
        q.w_embed = w;
        EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "embed_weight") && has(msg, "finite, not 0 and at most 4"));
    }
    for (float w : {4.5f, NAN, -INFINITY}) {
        q = good_query();
        q.w_audio = w;
        EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "audio_weight") && has(msg, "finite and at most 4"));
    }
    for (int64_t row : {int64_t{-1}, int64_t{100}, int64_t{1} << 40}) {   // w_audio != 0 needs a row of the handle, or audio by value
        q = good_query();
        q.w_audio = 1.0f;
        q.audio_row = row;
        EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "needs audio by value or a valid audio_row"));
        float audio[12] = {};
        q.audio = audio;
        EXPECT(!refuse_query(q, good_result(), msg, sizeof msg, &r) && r.use_audio && r.audio == audio && r.audio_row == -1);
    }
    q = good_query();
    q.w_audio = -4.0f;
    q.audio_row = 99;
    EXPECT(!refuse_query(q, good_result(), msg, sizeof msg, &r) && r.use_audio && r.audio_row == 99 && r.audio == nullptr);
    q.w_audio = 0.0f;   // (the row is not looked at)
    q.audio_row = 1000;
    EXPECT(!refuse_query(q, good_result(), msg, sizeof msg, &r) && !r.use_audio);
    for (int topn : {0, -3, 1025}) {
        q = good_query();
        q.topn = topn;
        EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "out of [1, 1024]"));
    }
    for (int topn : {1, 129, 1024}) {
        q = good_query();
        q.topn = topn;
        EXPECT(!refuse_query(q, good_result(), msg, sizeof msg));
    }
    for (int L : {-1, 1025}) {
        q = good_query();
        q.n_exclude = L;
        q.exclude_dev = fake_ids;
        EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "n_exclude") && has(msg, "out of [0, 1024]"));
    }
    q = good_query();
    q.n_exclude = 5;
    EXPECT(refuse_query(q, good_result(), msg, sizeof msg) && has(msg, "null exclusion list with n_exclude 5"));
    q.exclude_dev = fake_ids;
    EXPECT(!refuse_query(q, good_result(), msg, sizeof msg, &r) && r.n_exclude == 5 && r.exclude_dev == fake_ids);
    q.n_exclude = 1024;
    EXPECT(!refuse_query(q, good_result(), msg, sizeof msg, &r) && r.n_exclude == 1024);
}

void check_users_refusals() {
    char msg[256];
    Users r;
    EXPECT(!refuse_users(good_users(), good_result(), msg, sizeof msg, &r));
    EXPECT(r.users_dev == fake_floats && r.n_users == 3 && r.topn == 10 && r.exclude_len == 0 && r.exclude_dev == nullptr && r.metric == MI355REC_EMBED_DOT);
    const size_t ends[] = {8, 16, 24, 28, 32, 36, 40, 44, 48};
    for (uint32_t size = 0; size <= 56; ++size) {
        auto q = good_users();
        q.size = size;
        const bool known = std::find(std::begin(ends), std::end(ends), size) != std::end(ends) || size == 4;
        const bool refused = refuse_users(q, good_result(), msg, sizeof msg);
        if (!known) EXPECT(refused && has(msg, "embed stream users of size") && has(msg, "not the end of a field of the 48 bytes"));
        else EXPECT(refused == (size < 44));   // (up to w_embed read as zero)
    }
    auto res = good_result();
    res.out_idx_dev = nullptr;
    EXPECT(refuse_users(good_users(), res, msg, sizeof msg) && has(msg, "null out_idx_dev"));
    auto q = good_users();
    q.flags = 1;
    EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "flags 0x1") && has(msg, "must be 0"));
    for (int n_users : {0, -1, 1025}) {
        q = good_users();
        q.n_users = n_users;
        EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "n_users") && has(msg, "out of [1, 1024]"));
    }
    for (int n_users : {1, 1024}) {
        q = good_users();
        q.n_users = n_users;
        EXPECT(!refuse_users(q, good_result(), msg, sizeof msg));
    }
    q = good_users();
    q.users_dev = nullptr;
    EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "null users_dev"));
    q.users_dev = reinterpret_cast<const float*>(uintptr_t{0x1008});
    EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "users_dev is not 16-byte aligned"));
    for (int topn : {0, 129, 1025}) {
        q = good_users();
        q.topn = topn;
        EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "out of [1, 128]"));
    }
    for (int topn : {1, 128}) {
        q = good_users();
        q.topn = topn;
        EXPECT(!refuse_users(q, good_result(), msg, sizeof msg));
    }
    for (int L : {-1, 1025}) {
        q = good_users();
        q.exclude_len = L;
        q.exclude_dev = fake_ids;
        EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "exclude_len") && has(msg, "out of [0, 1024]"));
    }
    q = good_users();
    q.exclude_len = 4;
    EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "null exclusion matrix with exclude_len 4"));
    q.exclude_dev = fake_ids;
    EXPECT(!refuse_users(q, good_result(), msg, sizeof msg, &r) && r.exclude_len == 4 && r.exclude_dev == fake_ids);
    q.exclude_len = 0;   // (a matrix of no columns excludes nothing)
    EXPECT(!refuse_users(q, good_result(), msg, sizeof msg, &r) && r.exclude_dev == nullptr);
    q = good_users();
    q.metric = 2;
    EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "metric 2"));
    for (float w : {0.0f, 4.5f, NAN}) {
        q = good_users();
        q.w_embed = w;
        EXPECT(refuse_users(q, good_result(), msg, sizeof msg) && has(msg, "embed_weight"));
    }
}

void check_tables() {
    char msg[256];
    const void* t = fake_floats;
    EXPECT(!invalid_table(t, 10, 16, MI355REC_EMBED_STREAM_FP32, 10, true, msg, sizeof msg));
    EXPECT(!invalid_table(t, 10, 128, MI355REC_EMBED_HALF_BF16, 10, false, msg, sizeof msg));
    EXPECT(!invalid_table(nullptr, 0, 64, MI355REC_EMBED_HALF_FP16, 0, true, msg, sizeof msg));
    EXPECT(invalid_table(t, 10, 16, 2, 10, true, msg, sizeof msg) && has(msg, "storage 2"));
    EXPECT(invalid_table(t, 10, 16, -2, 10, true, msg, sizeof msg) && has(msg, "storage -2"));
    EXPECT(invalid_table(t, 10, 24, MI355REC_EMBED_STREAM_FP32, 10, true, msg, sizeof msg) && has(msg, "embedding dim 24: 16, 32, 64 or 128"));
    EXPECT(invalid_table(t, 9, 16, MI355REC_EMBED_STREAM_FP32, 10, true, msg, sizeof msg) && has(msg, "table of 9 rows for a handle of 10 rows"));
    EXPECT(invalid_table(nullptr, 10, 16, MI355REC_EMBED_STREAM_FP32, 10, true, msg, sizeof msg) && has(msg, "null table"));
    const void* odd = reinterpret_cast<const void*>(uintptr_t{0x1008});
    EXPECT(invalid_table(odd, 10, 16, MI355REC_EMBED_STREAM_FP32, 10, true, msg, sizeof msg) && has(msg, "16-byte aligned"));
    EXPECT(!invalid_table(odd, 10, 16, MI355REC_EMBED_STREAM_FP32, 10, false, msg, sizeof msg));   // (a host table is copied)
}

// What the scans must answer for `local`: is it among the ids of this table, by the host libraries' own normalisation.
std::vector<uint32_t> sorted_distinct(const std::vector<int64_t>& ids, int64_t base, int64_t n) {
    std::vector<uint32_t> rows;
    for (int64_t id : ids)
        if (id >= base && id - base < n) rows.push_back(static_cast<uint32_t>(id - base));
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    return rows;
}

void check_one_list(const std::vector<int64_t>& ids, int64_t base, int64_t n) {
    const int L = static_cast<int>(ids.size());
    std::unique_ptr<uint32_t[]> out(new uint32_t[L ? L : 1]);   // exactly L words: a store past them is the sanitizer's
    prepare_list(ids.data(), L, base, n, out.get());
    EXPECT(std::is_sorted(out.get(), out.get() + L));
    // the multiset is the mapped ids'
    std::vector<uint32_t> mapped;
    for (int64_t id : ids) mapped.push_back(local_row(id, base, n));
    std::sort(mapped.begin(), mapped.end());
    EXPECT(std::equal(mapped.begin(), mapped.end(), out.get()));
    // membership by lower bound + equality is membership in the sorted distinct list, for every row near the list and the edges
    const std::vector<uint32_t> want = sorted_distinct(ids, base, n);
    std::vector<int64_t> probes = {0, 1, n - 1, n / 2};
    for (uint32_t r : want) probes.insert(probes.end(), {static_cast<int64_t>(r) - 1, static_cast<int64_t>(r), static_cast<int64_t>(r) + 1});
    for (int64_t p : probes) {
        if (p < 0 || p >= n) continue;
        const uint32_t local = static_cast<uint32_t>(p);
        EXPECT(excluded(out.get(), L, local) == std::binary_search(want.begin(), want.end(), local));
    }
    EXPECT(!excluded(out.get(), L, static_cast<uint32_t>(n)) || n >= (int64_t{1} << 32));   // (no row of the table: never asked, never found)
}

void check_prepare() {
    EXPECT(prepare_width(1) == 64 && prepare_width(64) == 64 && prepare_width(65) == 128 && prepare_width(1023) == 1024 && prepare_width(1024) == 1024);
    EXPECT(local_row(-1, 0, 10) == kNoRow && local_row(10, 0, 10) == kNoRow && local_row(9, 0, 10) == 9u && local_row(0, 0, 10) == 0u);
    EXPECT(local_row(5, 1000000, 10) == kNoRow && local_row(1000009, 1000000, 10) == 9u && local_row(1000010, 1000000, 10) == kNoRow);
    EXPECT(local_row(INT64_MIN, 1000000, 10) == kNoRow && local_row(INT64_MAX, 1000000, 10) == kNoRow && local_row(INT64_MAX, 0, 10) == kNoRow);
    std::mt19937_64 rng(7);
    for (int64_t base : {int64_t{0}, int64_t{1000000}}) {
        for (int64_t n : {int64_t{1}, int64_t{17}, int64_t{1024}, int64_t{1025}, int64_t{4097}, int64_t{65537}}) {
            // the hostile list of the GPU tests, a descending one, every row (up to 1024), all the same row, foreign ids only
            check_one_list({base + 1, base + 1, base + 3, base + n - 1, base + n, base + n + 9, (int64_t{1} << 31) + 1, int64_t{1} << 40, -1}, base, n);
            std::vector<int64_t> desc, every, same(1024, base + n - 1), foreign(300, base + n);
            for (int64_t r = std::min<int64_t>(n, 1000) - 1; r >= 0; --r) desc.push_back(base + r);
            for (int64_t r = 0; r < std::min<int64_t>(n, 1024); ++r) every.push_back(base + (r * 7919) % std::min<int64_t>(n, 1024));
            check_one_list(desc, base, n);
            check_one_list(every, base, n);
            check_one_list(same, base, n);
            check_one_list(foreign, base, n);
            if (base > 0) check_one_list({0, 1, n - 1, base - 1, base, base + n - 1}, base, n);   // local rows are not global ids
            for (int L : {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024}) {   // random, dense in duplicates and in foreign ids
                std::vector<int64_t> ids(static_cast<size_t>(L));
                for (auto& id : ids) {
                    const uint64_t x = rng();
                    id = (x & 7) == 0 ? -static_cast<int64_t>(x >> 40) : base - 3 + static_cast<int64_t>((x >> 8) % static_cast<uint64_t>(n + 6));
                }
                check_one_list(ids, base, n);
            }
        }
    }
}

void check_finish() {
    std::mt19937 rng(11);
    for (int topn : {1, 10, 128, 257, 1024}) {
        for (int eff : {0, 1, topn / 2, topn}) {
            for (int count : {0, 1, eff / 2, eff}) {
                if (count > eff) continue;
                std::vector<uint64_t> keys(static_cast<size_t>(eff), 0ull);
                for (int i = 0; i < count; ++i) {
                    const float v = i == 0 ? -0.0f : (i == 1 ? 1e-40f : static_cast<float>(static_cast<int>(rng() % 2001) - 1000) / 64.0f);
                    keys[static_cast<size_t>(i)] = mi355embed::key_of(v, (i % 3 == 0) ? 0xFFFFFFFEu - static_cast<uint32_t>(i) : rng());
                }
                std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
                int nonzero = 0;
                for (uint64_t k : keys) nonzero += k != 0ull;
                std::vector<int64_t> idx(static_cast<size_t>(topn), 77), want_idx(static_cast<size_t>(topn), 78);
                std::vector<float> score(static_cast<size_t>(topn), 7.0f), want_score(static_cast<size_t>(topn), 8.0f);
                int32_t c = -5;
                int want_c = -6;
                finish_keys(keys.data(), eff, topn, idx.data(), score.data(), &c);
                mi355rec_embed_result_t res{};
                res.size = sizeof res;
                res.out_idx = want_idx.data();
                res.out_score = want_score.data();
                res.out_count = &want_c;
                mi355embed::write_result(keys.data(), nonzero, topn, res);
                EXPECT(c == want_c && c == nonzero && idx == want_idx);
                EXPECT(std::memcmp(score.data(), want_score.data(), sizeof(float) * static_cast<size_t>(topn)) == 0);
                for (int i = c; i < topn; ++i) EXPECT(idx[static_cast<size_t>(i)] == -1 && score[static_cast<size_t>(i)] == 0.0f);
                // score and count are optional
                std::vector<int64_t> only(static_cast<size_t>(topn), 79);
                finish_keys(keys.data(), eff, topn, only.data(), nullptr, nullptr);
                EXPECT(only == want_idx);
            }
        }
    }
}

}  // namespace

int main() {
    check_layout();
    check_query_refusals();
    check_users_refusals();
    check_tables();
    check_prepare();
    check_finish();
    if (failures) {
        std::printf("embed_stream_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_stream_request.h: ok\n");
    return 0;
}
