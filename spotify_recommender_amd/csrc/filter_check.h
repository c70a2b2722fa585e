// filter_check.h — the argument checks of a feature filter (include/mi355rec_diag.h, "FEATURE FILTERS"), shared by the
// single handle (engine_playlist.hip.h) and the node handle (sharded.hip), which both report them as INVALID_ARG.
#pragma once

#include <cmath>
#include <cstdio>

#include "mi355rec_diag.h"

namespace mi355filter {

constexpr uint32_t kAllFeatures = (1u << MI355REC_DIM) - 1u;

// True when `f` (non-null) cannot be used; then msg[0..cap) says why.
inline bool invalid(const mi355rec_filter_t* f, char* msg, size_t cap) {
    if (f->active & ~kAllFeatures) {
        std::snprintf(msg, cap, "filter: active mask 0x%x names features beyond the %d columns", f->active, MI355REC_DIM);
        return true;
    }
    for (int j = 0; j < MI355REC_DIM; ++j) {
        if (!(f->active & (1u << j))) continue;
        if (std::isnan(f->lo[j]) || std::isnan(f->hi[j])) {
            std::snprintf(msg, cap, "filter: NaN bound on feature %d", j);
            return true;
        }
        if (f->lo[j] > f->hi[j]) {
            std::snprintf(msg, cap, "filter: feature %d has lo %g > hi %g", j, static_cast<double>(f->lo[j]), static_cast<double>(f->hi[j]));
            return true;
        }
    }
    return false;
}

// True when x (12 floats) passes `f` (null or active == 0: every row passes).
inline bool pass(const mi355rec_filter_t* f, const float* x) {
    if (!f) return true;
    for (int j = 0; j < MI355REC_DIM; ++j)
        if ((f->active & (1u << j)) && !(f->lo[j] <= x[j] && x[j] <= f->hi[j])) return false;
    return true;
}

}  // namespace mi355filter
