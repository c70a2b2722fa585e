// bucket_sample.h — the host half of the DIRECTION-BUCKETED SAMPLE of the 8-bit scan (replica_q8.hip.h, "the bucketed
// sample"): ordering the base rows by (bucket, row) and cutting the order into regions.  Plain C++ with no device or
// engine type in it, so that tests/bucket_sample_check.cpp can run it stand-alone under the sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mi355 {

constexpr int kBucketRegionRows = 2048;   // rows of a region: one 48 B load of three per lane of a 512-thread workgroup

struct BucketOrder {
    std::vector<int32_t> rows;         // regions x kBucketRegionRows local rows in (bucket, row) order; the tail of the last region is -1
    std::vector<int32_t> region_tab;   // per region: the bucket of its first entry, the bucket of its last REAL entry
    int regions = 0;
};

// base_rows[i] (ascending, distinct) is the local row of base entry i and bucket[i] in [0, n_buckets) its bucket.  A
// stable counting sort by bucket: inside a bucket the rows keep their ascending order.  False (and `out` empty) when
// an argument is out of range — a bucket id outside [0, n_buckets) would index past the histogram.
inline bool bucket_sample_sort(const int32_t* base_rows, const int32_t* bucket, int64_t m, int n_buckets, BucketOrder& out) {
    out.rows.clear();
    out.region_tab.clear();
    out.regions = 0;
    if (m <= 0 || n_buckets <= 0 || !base_rows || !bucket) return false;
    std::vector<int64_t> start(static_cast<size_t>(n_buckets) + 1, 0);
    for (int64_t i = 0; i < m; ++i) {
        if (bucket[i] < 0 || bucket[i] >= n_buckets) return false;
        ++start[static_cast<size_t>(bucket[i]) + 1];
    }
    for (int b = 0; b < n_buckets; ++b) start[static_cast<size_t>(b) + 1] += start[static_cast<size_t>(b)];
    const int64_t regions = (m + kBucketRegionRows - 1) / kBucketRegionRows;
    out.rows.assign(static_cast<size_t>(regions) * kBucketRegionRows, -1);
    std::vector<int32_t> sorted_bucket(static_cast<size_t>(m));
    for (int64_t i = 0; i < m; ++i) {
        const int64_t at = start[static_cast<size_t>(bucket[i])]++;
        out.rows[static_cast<size_t>(at)] = base_rows[i];
        sorted_bucket[static_cast<size_t>(at)] = bucket[i];
    }
    out.region_tab.resize(static_cast<size_t>(regions) * 2);
    for (int64_t g = 0; g < regions; ++g) {
        const int64_t first = g * kBucketRegionRows;
        const int64_t last = (first + kBucketRegionRows < m ? first + kBucketRegionRows : m) - 1;
        out.region_tab[static_cast<size_t>(2 * g)] = sorted_bucket[static_cast<size_t>(first)];
        out.region_tab[static_cast<size_t>(2 * g + 1)] = sorted_bucket[static_cast<size_t>(last)];
    }
    out.regions = static_cast<int>(regions);
    return true;
}

}  // namespace mi355
