// weights_check.h — the argument checks of a weighted playlist (include/mi355rec_diag.h, "WEIGHTED PLAYLISTS") and its
// divisor W, shared by the single handle (engine_playlist.hip.h), the node handle (sharded.hip) and the CPU backend.
#pragma once

#include <cmath>
#include <cstdio>

#include "mi355rec_diag.h"

namespace mi355weights {

constexpr float kMaxWeight = 1e6f;   // |w_k| above this: INVALID_ARG
constexpr float kMinSum = 1e-6f;     // W below this (all weights zero included): INVALID_ARG

// W = fl(...fl(|w_0| + |w_1|) + ... + |w_{k-1}|) in fp32, member order (additions only: nothing a compiler could fuse).
inline float sum_abs(const float* w, int k) {
    float s = std::fabs(w[0]);
    for (int m = 1; m < k; ++m) s = s + std::fabs(w[m]);
    return s;
}

// True when w[0..k) (non-null, k >= 1) cannot be used; then msg[0..cap) says why.
inline bool invalid(const float* w, int k, char* msg, size_t cap) {
    for (int m = 0; m < k; ++m) {
        if (!std::isfinite(w[m])) {
            std::snprintf(msg, cap, "weights: weight %d is not finite", m);
            return true;
        }
        if (std::fabs(w[m]) > kMaxWeight) {
            std::snprintf(msg, cap, "weights: |weight %d| = %g exceeds %g", m, static_cast<double>(std::fabs(w[m])),
                          static_cast<double>(kMaxWeight));
            return true;
        }
    }
    const float s = sum_abs(w, k);
    if (s < kMinSum) {
        std::snprintf(msg, cap, "weights: the sum of |weights| %g is below %g (all weights zero?)", static_cast<double>(s),
                      static_cast<double>(kMinSum));
        return true;
    }
    return false;
}

}  // namespace mi355weights
