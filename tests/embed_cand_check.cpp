// embed_cand_check.cpp — csrc/embed_cand_request.h as a stand-alone program (its own main), built by
// tests/test_embed_cand_cpu.py with -fsanitize=address,undefined: the request and the two results read from heap buffers
// of exactly their size, every refusal with its text, and the plain statements of the ID MAPPING and of the CLAIM ("one
// entry per distinct in-table row keeps its row, the bitmap is all zero again behind the owners") against std::sort +
// std::unique on hostile lists.  No pointer named *_dev is dereferenced by the header: the ones given here are small
// integers on purpose.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "embed_cand_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using namespace mi355embedcand;

const float* fake_floats = reinterpret_cast<const float*>(uintptr_t{0x1000});     // "device" pointers: aligned, never read
const int64_t* fake_ids = reinterpret_cast<const int64_t*>(uintptr_t{0x2000});
int64_t* fake_idx = reinterpret_cast<int64_t*>(uintptr_t{0x3000});
float* fake_out = reinterpret_cast<float*>(uintptr_t{0x4000});

bool has(const char* msg, const char* text) { return std::strstr(msg, text) != nullptr; }

mi355rec_embed_stream_result_t good_result() {
    mi355rec_embed_stream_result_t res{};
    res.size = sizeof res;
    res.out_idx_dev = fake_idx;
    return res;
}

mi355rec_embed_cand_scores_t good_scores() {
    mi355rec_embed_cand_scores_t res{};
    res.size = sizeof res;
    res.out_v_dev = fake_out;
    return res;
}

mi355rec_embed_cand_query_t good_query() {
    mi355rec_embed_cand_query_t q{};
    q.size = sizeof q;
    q.user_dev = fake_floats;
    q.candidates_dev = fake_ids;
    q.n_candidates = 500;
    q.audio_row = -1;
    q.topn = 10;
    q.metric = MI355REC_EMBED_COSINE;
    q.w_embed = 1.0f;
    return q;
}

// The request and the result from heap copies of exactly their `size` bytes, as a caller with an older header hands them over.
template <class Res>
std::unique_ptr<char[]> heap_copy(const Res& x) {
    const size_t n = std::max<size_t>(x.size, sizeof x.size);   // (`size` itself is always there)
    std::unique_ptr<char[]> b(new char[n]);
    std::memcpy(b.get(), &x, std::min(n, sizeof x));
    return b;
}

bool refuse_rank(const mi355rec_embed_cand_query_t& q, const mi355rec_embed_stream_result_t& res, char* msg, size_t cap, Query* out = nullptr,
                 int64_t n_rows = 100) {
    const auto qb = heap_copy(q), rb = heap_copy(res);
    mi355rec_embed_cand_query_t full;
    mi355rec_embed_stream_result_t fres;
    Query r;
    msg[0] = 0;
    const bool refused = from_cand_rank(reinterpret_cast<const mi355rec_embed_cand_query_t*>(qb.get()),
                                        reinterpret_cast<const mi355rec_embed_stream_result_t*>(rb.get()), n_rows, &full, &fres, &r, msg, cap);
    if (out) *out = r;
    return refused;
}

bool refuse_scores(const mi355rec_embed_cand_query_t& q, const mi355rec_embed_cand_scores_t& res, char* msg, size_t cap, Query* out = nullptr,
                   int64_t n_rows = 100) {
    const auto qb = heap_copy(q), rb = heap_copy(res);
    mi355rec_embed_cand_query_t full;
    mi355rec_embed_cand_scores_t fres;
    Query r;
    msg[0] = 0;
    const bool refused = from_cand_scores(reinterpret_cast<const mi355rec_embed_cand_query_t*>(qb.get()),
                                          reinterpret_cast<const mi355rec_embed_cand_scores_t*>(rb.get()), n_rows, &full, &fres, &r, msg, cap);
    if (out) *out = r;
    return refused;
}

void check_layout() {
    using Q = mi355rec_embed_cand_query_t;
    using S = mi355rec_embed_cand_scores_t;
    using I = mi355rec_embed_cand_info_t;
    EXPECT(sizeof(Q) == 80 && offsetof(Q, user_dev) == 8 && offsetof(Q, audio) == 16 && offsetof(Q, candidates_dev) == 24 && offsetof(Q, exclude_dev) == 32);
    EXPECT(offsetof(Q, audio_row) == 40 && offsetof(Q, n_candidates) == 48 && offsetof(Q, n_exclude) == 56 && offsetof(Q, topn) == 60);
    EXPECT(offsetof(Q, metric) == 64 && offsetof(Q, w_audio) == 68 && offsetof(Q, w_embed) == 72 && offsetof(Q, reserved) == 76);
    EXPECT(sizeof(S) == 32 && offsetof(S, out_v_dev) == 8 && offsetof(S, out_c_dev) == 16 && offsetof(S, out_flag_dev) == 24);
    EXPECT(sizeof(I) == 96 && offsetof(I, table_dev) == 40 && offsetof(I, borrowed) == 76 && offsetof(I, max_candidates) == 80);
    EXPECT(offsetof(I, rank_launches) == 84 && offsetof(I, scores_call_launches) == 88 && offsetof(I, reserved) == 92);
    EXPECT(offsetof(I, pass_users) == offsetof(mi355rec_embed_stream_info_t, pass_users) && offsetof(I, launches) == offsetof(mi355rec_embed_stream_info_t, launches));
    EXPECT(MI355REC_EMBED_CAND_MAX == 1048576 && MI355REC_EMBED_CAND_MAX_EXCLUDE == MI355REC_EMBED_STREAM_MAX_EXCLUDE);
}

void check_refusals() {
    char msg[256];
    Query r;
    EXPECT(!refuse_rank(good_query(), good_result(), msg, sizeof msg, &r));
    EXPECT(r.user_dev == fake_floats && r.candidates_dev == fake_ids && r.n_candidates == 500 && r.topn == 10 && r.n_exclude == 0 && !r.use_audio);
    EXPECT(!refuse_scores(good_query(), good_scores(), msg, sizeof msg, &r) && r.topn == 0 && r.n_exclude == 0 && r.exclude_dev == nullptr);
    {
        mi355rec_embed_cand_query_t full;
        mi355rec_embed_stream_result_t fres;
        mi355rec_embed_cand_scores_t fsc;
        const auto q = good_query();
        const auto res = good_result();
        const auto sc = good_scores();
        EXPECT(from_cand_rank(nullptr, &res, 100, &full, &fres, &r, msg, sizeof msg) && has(msg, "null argument"));
        EXPECT(from_cand_rank(&q, nullptr, 100, &full, &fres, &r, msg, sizeof msg) && has(msg, "null argument"));
        EXPECT(from_cand_scores(nullptr, &sc, 100, &full, &fsc, &r, msg, sizeof msg) && has(msg, "null argument"));
        EXPECT(from_cand_scores(&q, nullptr, 100, &full, &fsc, &r, msg, sizeof msg) && has(msg, "null argument"));
    }
    // sizes: the end of every field is served; anything else, 0 and more than the struct are refused
    const size_t ends[] = {4, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80};
    for (uint32_t size = 0; size <= 88; ++size) {
        auto q = good_query();
        q.size = size;
        const bool known = std::find(std::begin(ends), std::end(ends), size) != std::end(ends);
        const bool refused = refuse_rank(q, good_result(), msg, sizeof msg);
        if (!known) EXPECT(refused && has(msg, "embed cand query of size") && has(msg, "not the end of a field of the 80 bytes"));
        else if (size < 16) EXPECT(refused && has(msg, "null user_dev"));   // (a struct that ends before user_dev reads it as zero)
        else if (size < 76) EXPECT(refused && has(msg, "embed_weight 0"));   // (n_candidates read as zero asks for no list; w_embed read as zero)
        else EXPECT(!refused);
    }
    for (uint32_t size : {0u, 7u, 12u, 20u, 31u, 33u, 40u}) {
        auto res = good_result();
        res.size = size;
        EXPECT(refuse_rank(good_query(), res, msg, sizeof msg) && has(msg, "embed stream result of size"));
        auto sc = good_scores();
        sc.size = size;
        EXPECT(refuse_scores(good_query(), sc, msg, sizeof msg) && has(msg, "embed cand scores of size") && has(msg, "32 bytes"));
    }
    for (uint32_t size : {4u, 8u, 16u, 24u, 32u}) {   // out_v_dev ends at 16: shorter reads it as null; c and the flag are optional
        auto sc = good_scores();
        sc.size = size;
        EXPECT(refuse_scores(good_query(), sc, msg, sizeof msg) == (size < 16u));
        if (size < 16u) EXPECT(has(msg, "null out_v_dev with n_candidates 500"));
    }
    auto res = good_result();
    res.out_idx_dev = nullptr;
    EXPECT(refuse_rank(good_query(), res, msg, sizeof msg) && has(msg, "null out_idx_dev"));
    res = good_result();
    res.reserved = 1;
    EXPECT(refuse_rank(good_query(), res, msg, sizeof msg) && has(msg, "reserved 0x1"));
    auto sc = good_scores();
    sc.reserved = 3;
    EXPECT(refuse_scores(good_query(), sc, msg, sizeof msg) && has(msg, "reserved 0x3 in an embed cand scores result: must be 0"));
    sc = good_scores();
    sc.out_v_dev = nullptr;
    EXPECT(refuse_scores(good_query(), sc, msg, sizeof msg) && has(msg, "null out_v_dev"));
    auto q = good_query();
    q.n_candidates = 0;   // (an empty list writes nothing: no output is asked for)
    q.candidates_dev = nullptr;
    EXPECT(!refuse_scores(q, sc, msg, sizeof msg, &r) && r.n_candidates == 0);
    EXPECT(!refuse_rank(q, good_result(), msg, sizeof msg, &r) && r.n_candidates == 0);

    q = good_query();
    q.flags = 2;
    EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "flags 0x2") && has(msg, "must be 0"));
    EXPECT(refuse_scores(q, good_scores(), msg, sizeof msg) && has(msg, "flags 0x2"));
    q = good_query();
    q.reserved = 7;
    EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "reserved 0x7"));
    q = good_query();
    q.user_dev = nullptr;
    EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "null user_dev") && has(msg, "members by rows are not served"));
    q = good_query();
    q.user_dev = reinterpret_cast<const float*>(uintptr_t{0x1004});
    EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "user_dev is not 16-byte aligned"));
    EXPECT(refuse_scores(q, good_scores(), msg, sizeof msg) && has(msg, "user_dev is not 16-byte aligned"));
    q = good_query();
    q.candidates_dev = nullptr;
    EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "null candidate list with n_candidates 500"));
    for (int64_t m : {int64_t{-1}, INT64_MIN, int64_t{MI355REC_EMBED_CAND_MAX} + 1, INT64_MAX}) {
        q = good_query();
        q.n_candidates = m;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "n_candidates") && has(msg, "out of [0, 1048576]"));
        EXPECT(refuse_scores(q, good_scores(), msg, sizeof msg) && has(msg, "out of [0, 1048576]"));
    }
    q = good_query();
    q.n_candidates = MI355REC_EMBED_CAND_MAX;
    EXPECT(!refuse_rank(q, good_result(), msg, sizeof msg, &r) && r.n_candidates == 1048576);
    for (int metric : {-1, 2}) {
        q = good_query();
        q.metric = metric;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "MI355REC_EMBED_COSINE (0) or MI355REC_EMBED_DOT (1)"));
    }
    for (float w : {0.0f, -0.0f, 4.5f, -4.5f, NAN, INFINITY}) {
        q = good_query();
        q.w_embed = w;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "embed_weight") && has(msg, "finite, not 0 and at most 4"));
        EXPECT(refuse_scores(q, good_scores(), msg, sizeof msg) && has(msg, "embed_weight"));
    }
    for (float w : {4.5f, NAN, -INFINITY}) {
        q = good_query();
        q.w_audio = w;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "audio_weight") && has(msg, "finite and at most 4"));
    }
    for (int64_t row : {int64_t{-1}, int64_t{100}, int64_t{1} << 40}) {   // w_audio != 0 needs a row of the handle, or audio by value
        q = good_query();
        q.w_audio = 1.0f;
        q.audio_row = row;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "needs audio by value or a valid audio_row"));
        float audio[12] = {};
        q.audio = audio;
        EXPECT(!refuse_rank(q, good_result(), msg, sizeof msg, &r) && r.use_audio && r.audio == audio && r.audio_row == -1);
    }
    q = good_query();
    q.w_audio = -4.0f;
    q.audio_row = 99;
    EXPECT(!refuse_scores(q, good_scores(), msg, sizeof msg, &r) && r.use_audio && r.audio_row == 99 && r.audio == nullptr);
    for (int topn : {0, -3, 1025}) {
        q = good_query();
        q.topn = topn;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "out of [1, 1024]"));
        EXPECT(!refuse_scores(q, good_scores(), msg, sizeof msg));   // (not read)
    }
    for (int L : {-1, 1025}) {
        q = good_query();
        q.n_exclude = L;
        q.exclude_dev = fake_ids;
        EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "n_exclude") && has(msg, "out of [0, 1024]"));
        EXPECT(!refuse_scores(q, good_scores(), msg, sizeof msg, &r) && r.n_exclude == 0);   // (not read)
    }
    q = good_query();
    q.n_exclude = 5;
    EXPECT(refuse_rank(q, good_result(), msg, sizeof msg) && has(msg, "null exclusion list with n_exclude 5"));
    q.exclude_dev = fake_ids;
    q.n_exclude = 1024;
    EXPECT(!refuse_rank(q, good_result(), msg, sizeof msg, &r) && r.n_exclude == 1024 && r.exclude_dev == fake_ids);
}

// What the claim must leave: the sorted distinct in-table rows of the list, by the host libraries' own normalisation.
std::vector<uint32_t> sorted_distinct(const std::vector<int64_t>& ids, int64_t base, int64_t n) {
    std::vector<uint32_t> rows;
    for (int64_t id : ids)
        if (id >= base && id - base < n) rows.push_back(static_cast<uint32_t>(id - base));
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    return rows;
}

void check_one_list(const std::vector<int64_t>& ids, int64_t base, int64_t n) {
    const int64_t m = static_cast<int64_t>(ids.size());
    const size_t words = static_cast<size_t>(claim_words(n));
    std::unique_ptr<uint32_t[]> bitmap(new uint32_t[words]());            // exactly the words of the table, all zero
    std::unique_ptr<uint32_t[]> rows(new uint32_t[m ? m : 1]);           // exactly m words: a store past them is the sanitizer's
    claim_list(ids.data(), m, base, n, bitmap.get(), rows.get());
    std::vector<uint32_t> kept;
    for (int64_t i = 0; i < m; ++i) {
        const uint32_t mapped = local_row(ids[static_cast<size_t>(i)], base, n);
        EXPECT(rows[i] == kNoRow || rows[i] == mapped);   // an entry keeps its own row or none
        if (rows[i] != kNoRow) kept.push_back(rows[i]);
    }
    std::sort(kept.begin(), kept.end());
    const std::vector<uint32_t> want = sorted_distinct(ids, base, n);
    EXPECT(kept == want);   // one claim per distinct in-table row: no row twice, none missing
    size_t bits = 0;
    for (size_t w = 0; w < words; ++w) bits += static_cast<size_t>(__builtin_popcount(bitmap[w]));
    EXPECT(bits == want.size());
    clear_claims(rows.get(), m, bitmap.get());
    for (size_t w = 0; w < words; ++w) EXPECT(bitmap[w] == 0u);   // all zero at rest
}

void check_claims() {
    EXPECT(claim_words(0) == 0 && claim_words(1) == 1 && claim_words(32) == 1 && claim_words(33) == 2 && claim_words(65537) == 2049);
    EXPECT(local_row(INT64_MIN, 1000000, 10) == kNoRow && local_row(INT64_MAX, 1000000, 10) == kNoRow && local_row(INT64_MAX, 0, 10) == kNoRow);
    EXPECT(local_row(999999, 1000000, 10) == kNoRow && local_row(1000010, 1000000, 10) == kNoRow && local_row(1000009, 1000000, 10) == 9u);
    EXPECT(gather_grid(1, 512, 129) == 1 && gather_grid(511, 512, 129) == 1 && gather_grid(512, 512, 129) == 1 && gather_grid(513, 512, 129) == 2);
    EXPECT(gather_grid(129 * 512 + 1, 512, 129) == 129 && gather_grid(1 << 20, 64, 2048) == 2048 && gather_grid(1 << 20, 1024, 1) == 1);
    std::mt19937_64 rng(7);
    for (int64_t base : {int64_t{0}, int64_t{1000000}}) {
        for (int64_t n : {int64_t{1}, int64_t{17}, int64_t{32}, int64_t{33}, int64_t{4097}, int64_t{65537}}) {
            check_one_list({}, base, n);
            check_one_list({-1, INT64_MIN, INT64_MAX, base - 1, base + n, base + n + 9, (int64_t{1} << 31) + 1, int64_t{1} << 40}, base, n);   // no id inside
            check_one_list({base + n - 1, -1, base, INT64_MIN, base + n - 1, INT64_MAX, base - 1, base + n, base, base + n / 2}, base, n);
            std::vector<int64_t> desc, twice, same(5000, base + n - 1);
            for (int64_t r = n - 1; r >= 0; --r) desc.push_back(base + r);
            for (int64_t r = 0; r < 2 * n; ++r) twice.push_back(base + (r * 7919) % n);
            check_one_list(desc, base, n);
            check_one_list(twice, base, n);
            check_one_list(same, base, n);   // every entry the same row
            if (base > 0) check_one_list({0, 1, n - 1, base - 1, base, base + n - 1}, base, n);   // local rows are not global ids
            for (int m : {1, 2, 63, 64, 65, 1023, 1025, 20000}) {   // random, dense in duplicates and in foreign ids
                std::vector<int64_t> ids(static_cast<size_t>(m));
                for (auto& id : ids) {
                    const uint64_t x = rng();
                    id = (x & 7) == 0 ? -static_cast<int64_t>(x >> 40) : base - 3 + static_cast<int64_t>((x >> 8) % static_cast<uint64_t>(n + 6));
                }
                check_one_list(ids, base, n);
            }
        }
    }
}

// `embed_cand_check claim IDS N ROW_BASE OUT`: claim_list over the int64 ids of the file IDS (a table of N rows from
// ROW_BASE on), its rows_out written to OUT as uint32 words; the bitmap must be all zero behind clear_claims.  The buffers
// are heap blocks of exactly their size, as in check_one_list.  (tests/test_embed_cand_steady_cpu.py holds its own
// statement of what a workgroup meets against this one.)
int claim_file(const char* ids_path, int64_t n, int64_t base, const char* out_path) {
    std::FILE* f = std::fopen(ids_path, "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    const int64_t m = bytes / static_cast<long>(sizeof(int64_t));
    std::unique_ptr<int64_t[]> ids(new int64_t[m ? m : 1]);
    const size_t got = std::fread(ids.get(), sizeof(int64_t), static_cast<size_t>(m), f);
    std::fclose(f);
    if (got != static_cast<size_t>(m) || n < 0) return 2;
    const size_t words = static_cast<size_t>(claim_words(n));
    std::unique_ptr<uint32_t[]> bitmap(new uint32_t[words ? words : 1]());
    std::unique_ptr<uint32_t[]> rows(new uint32_t[m ? m : 1]);
    claim_list(ids.get(), m, base, n, bitmap.get(), rows.get());
    clear_claims(rows.get(), m, bitmap.get());
    for (size_t w = 0; w < words; ++w) EXPECT(bitmap[w] == 0u);
    std::FILE* out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const size_t put = std::fwrite(rows.get(), sizeof(uint32_t), static_cast<size_t>(m), out);
    std::fclose(out);
    return (put == static_cast<size_t>(m) && failures == 0) ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && std::strcmp(argv[1], "claim") == 0) return claim_file(argv[2], std::atoll(argv[3]), std::atoll(argv[4]), argv[5]);
    check_layout();
    check_refusals();
    check_claims();
    if (failures) {
        std::printf("embed_cand_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_cand_request.h: ok\n");
    return 0;
}
