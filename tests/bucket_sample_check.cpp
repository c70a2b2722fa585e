// Stand-alone check of csrc/bucket_sample.h (the host sort of the 8-bit scan's bucketed sample), built with
// -fsanitize=address,undefined by tests/test_bucket_sample_cpu.py and run as its own process.
//   bucket_sample_check                      the fixed cases below
//   bucket_sample_check sort IN OUT          IN: int64 m, int64 n_buckets, int32 rows[m], int32 bucket[m]
//                                            OUT: int32 ok, int32 regions, int32 rows[regions * 2048], int32 tab[regions * 2]
#include "bucket_sample.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

using mi355::BucketOrder;
using mi355::bucket_sample_sort;
using mi355::kBucketRegionRows;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// permutation of the input, buckets non-decreasing, rows ascending inside a bucket, padding -1, the region table
static void check_order(const std::vector<int32_t>& rows, const std::vector<int32_t>& bucket, int n_buckets, const char* name) {
    const int64_t m = static_cast<int64_t>(rows.size());
    BucketOrder o;
    const bool ok = bucket_sample_sort(rows.data(), bucket.data(), m, n_buckets, o);
    CHECK(ok);
    if (!ok) return;
    const int64_t regions = (m + kBucketRegionRows - 1) / kBucketRegionRows;
    CHECK(o.regions == regions);
    CHECK(static_cast<int64_t>(o.rows.size()) == regions * kBucketRegionRows);
    CHECK(static_cast<int64_t>(o.region_tab.size()) == regions * 2);
    std::vector<int32_t> got(o.rows.begin(), o.rows.begin() + m), want(rows);
    for (int64_t i = m; i < regions * kBucketRegionRows; ++i) CHECK(o.rows[static_cast<size_t>(i)] == -1);
    std::vector<int32_t> of_row(static_cast<size_t>(*std::max_element(rows.begin(), rows.end())) + 1, -1);
    for (int64_t i = 0; i < m; ++i) of_row[static_cast<size_t>(rows[static_cast<size_t>(i)])] = bucket[static_cast<size_t>(i)];
    for (int64_t i = 1; i < m; ++i) {
        const int32_t b0 = of_row[static_cast<size_t>(got[static_cast<size_t>(i - 1)])], b1 = of_row[static_cast<size_t>(got[static_cast<size_t>(i)])];
        CHECK(b0 <= b1);
        if (b0 == b1) CHECK(got[static_cast<size_t>(i - 1)] < got[static_cast<size_t>(i)]);
    }
    for (int64_t g = 0; g < regions; ++g) {
        const int64_t first = g * kBucketRegionRows, last = std::min<int64_t>(first + kBucketRegionRows, m) - 1;
        CHECK(o.region_tab[static_cast<size_t>(2 * g)] == of_row[static_cast<size_t>(got[static_cast<size_t>(first)])]);
        CHECK(o.region_tab[static_cast<size_t>(2 * g + 1)] == of_row[static_cast<size_t>(got[static_cast<size_t>(last)])]);
    }
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    CHECK(got == want);
    if (failures) std::printf("  (case %s)\n", name);
}

static std::vector<int32_t> strided_rows(int64_t m, int stride) {
    std::vector<int32_t> r(static_cast<size_t>(m));
    for (int64_t i = 0; i < m; ++i) r[static_cast<size_t>(i)] = static_cast<int32_t>((i / 2048) * stride + i % 2048);
    return r;
}

static int fixed_cases() {
    uint32_t x = 12345u;
    auto rnd = [&]() { return x = x * 1664525u + 1013904223u; };
    {   // every row in one bucket
        const int64_t m = 3 * 2048;
        check_order(strided_rows(m, 5000), std::vector<int32_t>(static_cast<size_t>(m), 7), 16, "one bucket");
    }
    {   // empty buckets: only every fifth bucket is used
        const int64_t m = 4 * 2048;
        std::vector<int32_t> b(static_cast<size_t>(m));
        for (auto& v : b) v = static_cast<int32_t>(rnd() % 8) * 5;
        check_order(strided_rows(m, 4096), b, 40, "empty buckets");
    }
    {   // a base that is not a multiple of 2048 rows
        for (int64_t m : {int64_t(1), int64_t(2047), int64_t(2049), int64_t(5 * 2048 + 333)}) {
            std::vector<int32_t> b(static_cast<size_t>(m));
            for (auto& v : b) v = static_cast<int32_t>(rnd() % 11);
            check_order(strided_rows(m, 2052), b, 11, "ragged base");
        }
    }
    {   // one region
        const int64_t m = 2048;
        std::vector<int32_t> b(static_cast<size_t>(m));
        for (auto& v : b) v = static_cast<int32_t>(rnd() % 64);
        check_order(strided_rows(m, 2048), b, 64, "one region");
    }
    {   // refusals: a bucket out of range, nothing to sort
        std::vector<int32_t> r = {0, 1, 2}, b = {0, 3, 1};
        BucketOrder o;
        CHECK(!bucket_sample_sort(r.data(), b.data(), 3, 3, o) && o.rows.empty() && o.regions == 0);
        b[1] = -1;
        CHECK(!bucket_sample_sort(r.data(), b.data(), 3, 3, o));
        CHECK(!bucket_sample_sort(r.data(), b.data(), 0, 3, o));
        CHECK(!bucket_sample_sort(nullptr, b.data(), 3, 3, o));
    }
    if (!failures) std::printf("bucket_sample.h: ok\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "sort") {
        std::ifstream in(argv[2], std::ios::binary);
        int64_t head[2] = {0, 0};
        in.read(reinterpret_cast<char*>(head), sizeof head);
        if (!in || head[0] < 0 || head[0] > (int64_t(1) << 26)) return 2;
        std::vector<int32_t> rows(static_cast<size_t>(head[0])), bucket(static_cast<size_t>(head[0]));
        in.read(reinterpret_cast<char*>(rows.data()), static_cast<std::streamsize>(rows.size() * 4));
        in.read(reinterpret_cast<char*>(bucket.data()), static_cast<std::streamsize>(bucket.size() * 4));
        if (!in) return 2;
        BucketOrder o;
        const int32_t ok = bucket_sample_sort(rows.data(), bucket.data(), head[0], static_cast<int>(head[1]), o) ? 1 : 0;
        std::ofstream out(argv[3], std::ios::binary);
        const int32_t regions = o.regions;
        out.write(reinterpret_cast<const char*>(&ok), 4);
        out.write(reinterpret_cast<const char*>(&regions), 4);
        out.write(reinterpret_cast<const char*>(o.rows.data()), static_cast<std::streamsize>(o.rows.size() * 4));
        out.write(reinterpret_cast<const char*>(o.region_tab.data()), static_cast<std::streamsize>(o.region_tab.size() * 4));
        return out ? 0 : 2;
    }
    return fixed_cases();
}
