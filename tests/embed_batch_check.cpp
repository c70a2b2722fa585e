// embed_batch_check.cpp — csrc/embed_batch_request.h as a stand-alone program (its own main), built by
// tests/test_embed_batch_cpu.py with -fsanitize=address,undefined: the self-sized structs are read at every size from
// buffers of exactly that size, every refusal names its reason and touches nothing beyond what the caller declared, and
// the exclusion lists come out sorted, distinct, local and without foreign ids from buffers that end where the lists end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "embed_batch_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

using namespace mi355embed;

struct Case {
    std::vector<float> users = std::vector<float>(3 * 16, 1.0f);
    std::vector<int64_t> idx = std::vector<int64_t>(3 * 8);
    mi355rec_embed_batch_query_t q{};
    mi355rec_embed_batch_result_t res{};
    mi355rec_embed_batch_query_t full;
    mi355rec_embed_batch_result_t fres;
    BatchRequest r;
    char msg[256];
    Case() {
        q.size = sizeof q;
        q.users = users.data();
        q.n_users = 3;
        q.topn = 8;
        q.w_embed = 1.0f;
        res.size = sizeof res;
        res.out_idx = idx.data();
        msg[0] = 0;
    }
    bool refused() { return from_batch_query(&q, &res, &full, &fres, &r, msg, sizeof msg); }
    bool refused_with(const char* text) { return refused() && std::strstr(msg, text); }
};

void check_sizes() {
    Case c;
    for (uint32_t size = 0; size <= sizeof c.q + 8; ++size) {
        // the query in a heap buffer of exactly `size` bytes: a read past what the caller declared is a sanitizer report
        std::unique_ptr<unsigned char[]> buf(new unsigned char[size ? size : 1]);
        mi355rec_embed_batch_query_t tmp = c.q;
        tmp.size = size;
        std::memcpy(buf.get(), &tmp, std::min<size_t>(size, sizeof tmp));
        if (size < sizeof(uint32_t)) continue;   // (a struct that cannot hold its own size field is not a struct)
        const bool refused = from_batch_query(reinterpret_cast<const mi355rec_embed_batch_query_t*>(buf.get()), &c.res, &c.full, &c.fres, &c.r, c.msg,
                                              sizeof c.msg);
        const bool is_end = size == 4 || size == 8 || size == 16 || size == 24 || size == 32 || size == 36 || size == 40 || size == 44 || size == 48;
        if (!is_end) EXPECT(refused && std::strstr(c.msg, "not the end of a field"));   // 0, mid-field, too long
        if (size == 48) EXPECT(!refused && c.r.topn == 8 && c.r.n_users == 3 && c.r.users == c.users.data() && !c.r.exclude_offsets);
        if (is_end && size < 48) EXPECT(refused);   // (a later field is missing: no users, topn 0 or the zero weight)
        if (size == 44) EXPECT(std::strstr(c.msg, "embed_weight 0"));   // a shorter struct: later fields are zero
    }
    for (uint32_t size : {0u, 20u, 36u}) {
        Case d;   // the result, likewise: size 0, mid-field, too long
        const size_t len = std::max<size_t>(size, sizeof(uint32_t));
        std::unique_ptr<unsigned char[]> buf(new unsigned char[len]());
        d.res.size = size;
        std::memcpy(buf.get(), &d.res, std::min(len, sizeof d.res));
        EXPECT(from_batch_query(&d.q, reinterpret_cast<const mi355rec_embed_batch_result_t*>(buf.get()), &d.full, &d.fres, &d.r, d.msg, sizeof d.msg) &&
               std::strstr(d.msg, "embed batch result of size"));
    }
    Case n;
    EXPECT(from_batch_query(nullptr, &n.res, &n.full, &n.fres, &n.r, n.msg, sizeof n.msg));
    EXPECT(from_batch_query(&n.q, nullptr, &n.full, &n.fres, &n.r, n.msg, sizeof n.msg));
    char tiny[8];
    n.q.topn = 0;
    EXPECT(from_batch_query(&n.q, &n.res, &n.full, &n.fres, &n.r, tiny, sizeof tiny) && tiny[7] == 0);   // a message longer than its buffer
}

void check_refusals() {
    const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
    { Case c; EXPECT(!c.refused()); }
    { Case c; c.q.n_users = 0; EXPECT(c.refused_with("n_users 0 out of [1, 1024]")); }
    { Case c; c.q.n_users = 1025; EXPECT(c.refused_with("n_users 1025 out of [1, 1024]")); }
    { Case c; c.q.n_users = -1; EXPECT(c.refused_with("n_users -1 out of")); }
    { Case c; c.q.topn = 0; EXPECT(c.refused_with("topn 0 out of [1, 128]")); }
    { Case c; c.q.topn = 129; EXPECT(c.refused_with("topn 129 out of [1, 128]")); }
    { Case c; c.q.w_embed = 0.0f; EXPECT(c.refused_with("embed_weight 0: finite, not 0 and at most 4")); }
    { Case c; c.q.w_embed = nan; EXPECT(c.refused_with("embed_weight nan")); }
    { Case c; c.q.w_embed = inf; EXPECT(c.refused_with("embed_weight inf")); }
    { Case c; c.q.w_embed = 4.5f; EXPECT(c.refused_with("embed_weight 4.5")); }
    { Case c; c.q.w_embed = -4.0f; EXPECT(!c.refused() && c.r.w_embed == -4.0f); }
    { Case c; c.q.metric = 2; EXPECT(c.refused_with("metric 2 in an embed batch query")); }
    { Case c; c.q.metric = MI355REC_EMBED_DOT; EXPECT(!c.refused() && c.r.metric == MI355REC_EMBED_DOT); }
    { Case c; c.q.flags = 1; EXPECT(c.refused_with("flags 0x1 in an embed batch query")); }
    { Case c; c.q.users = nullptr; EXPECT(c.refused_with("null users")); }
    { Case c; c.res.out_idx = nullptr; EXPECT(c.refused_with("null out_idx")); }
    // the exclusion lists: both pointers or neither, offsets >= 0 and non-decreasing, at most 65536 ids per user
    std::unique_ptr<int64_t[]> ids(new int64_t[4]{5, 5, 6, 7});
    std::unique_ptr<int64_t[]> off(new int64_t[4]{0, 2, 2, 4});
    { Case c; c.q.exclude_global = ids.get(); EXPECT(c.refused_with("both or neither")); }
    { Case c; c.q.exclude_offsets = off.get(); EXPECT(c.refused_with("both or neither")); }
    { Case c; c.q.exclude_global = ids.get(); c.q.exclude_offsets = off.get(); EXPECT(!c.refused() && c.r.exclude == ids.get()); }
    { Case c; off[2] = 1; c.q.exclude_global = ids.get(); c.q.exclude_offsets = off.get(); EXPECT(c.refused_with("exclude_offsets decrease at user 1")); off[2] = 2; }
    { Case c; off[0] = -1; c.q.exclude_global = ids.get(); c.q.exclude_offsets = off.get(); EXPECT(c.refused_with("exclude_offsets[0] is -1")); off[0] = 0; }
    {
        // user 1 lists 65537 ids (never read by the checks: a buffer of that many, so that a read would be in bounds anyway)
        Case c;
        std::vector<int64_t> many(65537 + 2, 3);
        std::unique_ptr<int64_t[]> o(new int64_t[4]{0, 1, 1 + 65537, 2 + 65537});
        c.q.exclude_global = many.data();
        c.q.exclude_offsets = o.get();
        EXPECT(c.refused_with("user 1 excludes 65537 ids: at most 65536"));
        o[2] = 1 + 65536;
        EXPECT(!c.refused());
    }
}

void check_normalisation() {
    // three users: a full list with duplicates, foreign and negative ids; an EMPTY list; a full list again — a table of 100
    // rows that starts at global row 1000
    const int64_t base = 1000, n = 100;
    std::unique_ptr<int64_t[]> ids(new int64_t[11]{1050, 1001, 1050, 7, -3, 1100, (int64_t(1) << 31) + 1001, 1099,   // user 0
                                                  1000, 1000, 1002});                                                // user 2
    std::unique_ptr<int64_t[]> off(new int64_t[4]{0, 8, 8, 11});
    Case c;
    c.q.exclude_global = ids.get();
    c.q.exclude_offsets = off.get();
    EXPECT(!c.refused());
    std::vector<uint32_t> rows;
    std::vector<int64_t> offsets;
    normalise_exclusions(c.r, base, n, &rows, &offsets);
    EXPECT((offsets == std::vector<int64_t>{0, 3, 3, 5}));
    EXPECT((rows == std::vector<uint32_t>{1, 50, 99, 0, 2}));
    // the same ids without a row_base: only 7 is a row of the table
    normalise_exclusions(c.r, 0, n, &rows, &offsets);
    EXPECT((offsets == std::vector<int64_t>{0, 1, 1, 1}) && (rows == std::vector<uint32_t>{7}));
    // offsets that do not start at 0 skip what lies before them
    off[0] = 7;
    EXPECT(!c.refused());
    normalise_exclusions(c.r, base, n, &rows, &offsets);
    EXPECT((offsets == std::vector<int64_t>{0, 1, 1, 3}) && (rows == std::vector<uint32_t>{99, 0, 2}));
    // nothing excluded: offsets of zeros, no rows
    Case none;
    EXPECT(!none.refused());
    normalise_exclusions(none.r, base, n, &rows, &offsets);
    EXPECT(rows.empty() && (offsets == std::vector<int64_t>{0, 0, 0, 0}));
    // extreme ids do not overflow the subtraction
    std::unique_ptr<int64_t[]> ext(new int64_t[2]{std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()});
    std::unique_ptr<int64_t[]> eoff(new int64_t[4]{0, 2, 2, 2});
    Case x;
    x.q.exclude_global = ext.get();
    x.q.exclude_offsets = eoff.get();
    EXPECT(!x.refused());
    normalise_exclusions(x.r, base, n, &rows, &offsets);
    EXPECT(rows.empty());
}

void check_results() {
    // two users, topn 3: user 0 has two keys, user 1 none; scores and counts optional
    const uint64_t keys[2] = {key_of(0.5f, 7u), key_of(-0.0f, 9u)};
    std::unique_ptr<int64_t[]> idx(new int64_t[6]);
    std::unique_ptr<float[]> score(new float[6]);
    std::unique_ptr<int32_t[]> count(new int32_t[2]);
    mi355rec_embed_batch_result_t res{};
    res.out_idx = idx.get();
    res.out_score = score.get();
    res.out_count = count.get();
    write_batch_result(keys, 2, 3, 0, res);
    write_batch_result(nullptr, 0, 3, 1, res);
    EXPECT(idx[0] == 7 && idx[1] == 9 && idx[2] == -1 && idx[3] == -1 && idx[5] == -1);
    EXPECT(score[0] == 0.5f && score[1] == 0.0f && !std::signbit(score[1]) && score[2] == 0.0f && score[4] == 0.0f);
    EXPECT(count[0] == 2 && count[1] == 0);
    res.out_score = nullptr;
    res.out_count = nullptr;
    write_batch_result(keys, 1, 3, 1, res);
    EXPECT(idx[3] == 7 && idx[4] == -1);
}

}  // namespace

int main() {
    check_sizes();
    check_refusals();
    check_normalisation();
    check_results();
    if (failures) {
        std::printf("embed_batch_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_batch_request.h: ok\n");
    return 0;
}
