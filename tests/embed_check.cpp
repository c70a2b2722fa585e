// embed_check.cpp — csrc/embed_request.h and csrc/embed_cpu.cpp as a stand-alone program (its own main), built by
// tests/test_embed_cpu.py with -fsanitize=address,undefined: the self-sized structs are read at every legal size from
// buffers of exactly that size, the refusals touch nothing beyond them, and the CPU placement's query agrees with a
// brute-force statement of the contract over tables whose buffers end where the rows end.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <random>
#include <vector>

#include "embed_request.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

void check_sizes() {
    using namespace mi355embed;
    std::vector<float> user(16, 1.0f);
    std::vector<int64_t> idx(8);
    mi355rec_embed_query_t q{};
    q.size = sizeof q;
    q.user = user.data();
    q.topn = 8;
    q.w_embed = 1.0f;
    mi355rec_embed_result_t res{};
    res.size = sizeof res;
    res.out_idx = idx.data();
    char msg[256];
    for (uint32_t size = 0; size <= sizeof q + 8; ++size) {
        // the query in a heap buffer of exactly `size` bytes: a read past what the caller declared is a sanitizer report
        std::unique_ptr<unsigned char[]> buf(new unsigned char[size ? size : 1]);
        mi355rec_embed_query_t tmp = q;
        tmp.size = size;
        std::memcpy(buf.get(), &tmp, std::min<size_t>(size, sizeof tmp));
        if (size < sizeof(uint32_t)) continue;   // (a struct that cannot hold its own size field is not a struct)
        mi355rec_embed_query_t full;
        mi355rec_embed_result_t fres;
        Request r;
        const bool refused = from_query(reinterpret_cast<const mi355rec_embed_query_t*>(buf.get()), &res, true, 100, &full, &fres, &r, msg, sizeof msg);
        const bool is_end = size == 8 || size == 16 || size == 24 || size == 32 || size == 40 || size == 48 || size == 52 || size == 56 ||
                            size == 60 || size == 64 || size == 68 || size == 72 || size == 4;
        if (!is_end) EXPECT(refused && std::strstr(msg, "not the end of a field"));
        if (size == 72) EXPECT(!refused && r.topn == 8 && r.user == user.data() && !r.use_audio);
        if (is_end && size < 72) EXPECT(refused);   // (a later field is missing: no user, or topn 0, or the zero weight)
    }
    mi355rec_embed_query_t full;
    mi355rec_embed_result_t fres;
    Request r;
    EXPECT(from_query(nullptr, &res, true, 100, &full, &fres, &r, msg, sizeof msg));
    EXPECT(from_query(&q, nullptr, true, 100, &full, &fres, &r, msg, sizeof msg));
    EXPECT(!from_query(&q, nullptr, false, 100, &full, nullptr, &r, msg, sizeof msg));   // a _scores call has no result
    char tiny[8];
    q.topn = 0;
    EXPECT(from_query(&q, &res, true, 100, &full, &fres, &r, tiny, sizeof tiny) && tiny[7] == 0);   // a message longer than its buffer
    EXPECT(invalid_table(user.data(), 4, 12, 4, msg, sizeof msg) && invalid_table(user.data(), 4, 16, 5, msg, sizeof msg));
    EXPECT(invalid_table(nullptr, 4, 16, 4, msg, sizeof msg) && !invalid_table(nullptr, 0, 16, 0, msg, sizeof msg));
}

// The contract, one row at a time, with a tree written as a recursion instead of levels.
float tree_rec(const float* a, const float* b, int lo, int groups) {
    if (groups == 1) {
        float p = a[4 * lo] * b[4 * lo];
        p = p + a[4 * lo + 1] * b[4 * lo + 1];
        p = p + a[4 * lo + 2] * b[4 * lo + 2];
        return p + a[4 * lo + 3] * b[4 * lo + 3];
    }
    const float l = tree_rec(a, b, lo, groups / 2);
    const float r = tree_rec(a, b, lo + groups / 2, groups / 2);
    return l + r;
}

void check_queries() {
    using namespace mi355embed;
    std::mt19937 gen(7);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    std::uniform_real_distribution<float> ud(0.0f, 1.0f);
    for (int d : {16, 32, 64, 128})
        for (int64_t n : {int64_t(1), int64_t(5), int64_t(1000)}) {
            // heap buffers that end where the rows end
            std::unique_ptr<float[]> table(new float[n * d]), feats(new float[n * 12]);
            for (int64_t i = 0; i < n * d; ++i) table[i] = nd(gen);
            for (int64_t i = 0; i < n * 12; ++i) feats[i] = ud(gen);
            if (n >= 5) {
                std::memcpy(&table[3 * d], &table[1 * d], sizeof(float) * d);
                std::memcpy(&feats[3 * 12], &feats[1 * 12], sizeof(float) * 12);
                for (int j = 0; j < d; ++j) table[4 * d + j] = 1e19f;
                table[2 * d] = std::nanf("");
            }
            for (int64_t i = 0; i < n; ++i) {
                const float a = tree(&table[i * d], &table[(n - 1 - i) * d], d);
                const float b = tree_rec(&table[i * d], &table[(n - 1 - i) * d], 0, d / 4);
                EXPECT(std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)));
            }
            CpuTable t;
            t.table = table.get();
            t.n = n;
            t.dim = d;
            t.audio_rows = feats.get();
            std::vector<int64_t> rows = {0, n - 1, n / 2};
            std::vector<int64_t> excl = {0, 0, n + 3, -5, n - 1};
            for (int variant = 0; variant < 4; ++variant) {
                Request r;
                r.rows = rows.data();
                r.k = 3;
                r.metric = variant & 1;
                r.w_embed = variant & 2 ? -0.5f : 0.25f;
                r.w_audio = variant & 1 ? 0.0f : 1.0f;
                r.use_audio = r.w_audio != 0.0f;
                r.audio_row = n / 2;
                r.exclude = excl.data();
                r.n_exclude = static_cast<int>(excl.size());
                r.topn = 7;
                std::vector<float> v(n), c(n);
                cpu_scores(t, r, v.data(), c.data());
                std::vector<int64_t> idx(r.topn);
                std::vector<float> score(r.topn);
                int count = -1;
                mi355rec_embed_result_t res{};
                res.size = sizeof res;
                res.out_idx = idx.data();
                res.out_score = score.data();
                res.out_count = &count;
                EXPECT(cpu_query(t, r, res));
                std::vector<uint64_t> keys;
                for (int64_t i = 0; i < n; ++i)
                    if (std::isfinite(v[i]) && i != 0 && i != n - 1) keys.push_back(key_of(v[i], static_cast<uint32_t>(i)));
                std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
                const int want = static_cast<int>(std::min<size_t>(keys.size(), 7));
                EXPECT(count == want);
                for (int i = 0; i < r.topn; ++i) {
                    if (i < want) {
                        EXPECT(idx[i] == static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(keys[i]))));
                        EXPECT(score[i] == v[idx[i]]);
                    } else {
                        EXPECT(idx[i] == -1 && score[i] == 0.0f);
                    }
                }
            }
        }
}

}  // namespace

int main() {
    check_sizes();
    check_queries();
    if (failures) {
        std::printf("embed_request.h: %d failures\n", failures);
        return 1;
    }
    std::printf("embed_request.h: ok\n");
    return 0;
}
