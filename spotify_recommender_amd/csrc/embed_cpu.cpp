// embed_cpu.cpp — hybrid requests over an embedding table on a host WITHOUT a HIP device (include/mi355rec_embed.h, the
// CPU placement of mi355rec_embed_create_node): the contract of embed_request.h over host memory, rows split over OpenMP
// threads.  The audio side is the chain of cpu_backend.cpp (Recommender.cu:256-273: sequential j = 0..11, multiply and add
// rounded separately, `> 1e-8f`, the std::min / std::max clamp) over the catalogue's live host matrix.  Compiled by g++
// with -O3 -ffp-contract=off and without -ffast-math, as cpu_backend.cpp is.
#include <algorithm>
#include <functional>
#include <new>
#include <vector>

#include "embed_request.h"

namespace mi355embed {

namespace {

inline float audio_norm(const float* q) {
    float qn = 0.0f;
    for (int j = 0; j < MI355REC_DIM; ++j) qn += q[j] * q[j];
    return std::sqrt(qn);
}

inline float audio_score(const float* q, float qn, const float* f) {
    float dot = 0.0f;
    float norm = 0.0f;
    for (int j = 0; j < MI355REC_DIM; ++j) {
        dot += q[j] * f[j];
        norm += f[j] * f[j];
    }
    norm = std::sqrt(norm) * qn;
    if (norm > 1e-8f) return std::max(-1.0f, std::min(1.0f, dot / norm));
    return 0.0f;
}

// What every row's value needs, formed once per request.
struct Prepared {
    float u[MI355REC_EMBED_MAX_DIM];
    float nu = 0.0f;
    float q[MI355REC_DIM];
    float qn = 0.0f;
};

Prepared prepare(const CpuTable& t, const Request& r) {
    Prepared p;
    if (r.user) {
        std::memcpy(p.u, r.user, sizeof(float) * static_cast<size_t>(t.dim));
    } else {
        sum_members(r, t.dim, [&](int64_t row, float* out) { std::memcpy(out, t.table + row * t.dim, sizeof(float) * static_cast<size_t>(t.dim)); },
                    p.u);
    }
    p.nu = std::sqrt(tree(p.u, p.u, t.dim));
    if (r.use_audio) {
        std::memcpy(p.q, r.audio ? r.audio : t.audio_rows + r.audio_row * MI355REC_DIM, sizeof p.q);
        p.qn = audio_norm(p.q);
    }
    return p;
}

inline float value(const CpuTable& t, const Request& r, const Prepared& p, int64_t i, float* c_out) {
    const float c = similarity(t.table + i * t.dim, p.u, p.nu, t.dim, r.metric);
    if (c_out) *c_out = c;
    const float s = r.use_audio ? audio_score(p.q, p.qn, t.audio_rows + i * MI355REC_DIM) : 0.0f;
    return blend(r, s, c);
}

}  // namespace

void cpu_scores(const CpuTable& t, const Request& r, float* out_v, float* out_c) {
    const Prepared p = prepare(t, r);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < t.n; ++i) out_v[i] = value(t, r, p, i, out_c ? out_c + i : nullptr);
}

bool cpu_query(const CpuTable& t, const Request& r, const mi355rec_embed_result_t& res) {
    const Prepared p = prepare(t, r);
    std::vector<uint64_t> keys;
    try {
        keys.resize(static_cast<size_t>(t.n));
    } catch (const std::bad_alloc&) {
        return false;
    }
    uint64_t* const k = keys.data();
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < t.n; ++i) {
        const float v = value(t, r, p, i, nullptr);
        k[i] = std::isfinite(v) ? key_of(v, static_cast<uint32_t>(i)) : 0ull;
    }
    for (int i = 0; i < r.n_exclude; ++i)
        if (r.exclude[i] >= 0 && r.exclude[i] < t.n) k[r.exclude[i]] = 0ull;
    const size_t live = static_cast<size_t>(std::partition(keys.begin(), keys.end(), [](uint64_t x) { return x != 0ull; }) - keys.begin());
    const size_t take = std::min(live, static_cast<size_t>(r.topn));
    std::partial_sort(keys.begin(), keys.begin() + static_cast<std::ptrdiff_t>(take), keys.begin() + static_cast<std::ptrdiff_t>(live),
                      std::greater<uint64_t>());
    write_result(k, static_cast<int>(take), r.topn, res);
    return true;
}

}  // namespace mi355embed
