// embed_half_request.h — what libmi355rec_embed_half.so (include/mi355rec_embed_half.h) adds to embed_request.h on the
// host: the create checks of a half table and W(x), the exact fp32 value of a stored word, in integer arithmetic (the
// host statement the stand-alone check tests/embed_half_check.cpp holds against a table-free one; the kernels widen with
// the hardware conversion, csrc/embed_half.hip.h).  A request is embed_request.h's Request, unchanged.  Host code only.
#pragma once

#include "embed_request.h"
#include "mi355rec_embed_half.h"

namespace mi355embedhalf {

inline bool valid_storage(int storage) { return storage == MI355REC_EMBED_HALF_FP16 || storage == MI355REC_EMBED_HALF_BF16; }

// True when a half table cannot be served; then msg[0..cap) says why.
inline bool invalid_table(const uint16_t* words, int64_t n, int dim, int storage, int64_t handle_rows, char* msg, size_t cap) {
    if (!valid_storage(storage)) {
        std::snprintf(msg, cap, "storage %d: MI355REC_EMBED_HALF_FP16 (0) or MI355REC_EMBED_HALF_BF16 (1)", storage);
        return true;
    }
    if (!mi355embed::valid_dim(dim)) {
        std::snprintf(msg, cap, "embedding dim %d: 16, 32, 64 or 128 are supported (zero-pad other widths)", dim);
        return true;
    }
    if (n != handle_rows) {
        std::snprintf(msg, cap, "table of %lld rows for a handle of %lld rows", static_cast<long long>(n), static_cast<long long>(handle_rows));
        return true;
    }
    if (n > 0 && !words) {
        std::snprintf(msg, cap, "null table");
        return true;
    }
    return false;
}

// The bits of W(x) for an IEEE binary16 word: subnormals are normalised (exact), inf stays inf, a NaN stays a NaN.
inline uint32_t widen_fp16_bits(uint16_t h) {
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16;
    const uint32_t exp = (h >> 10) & 0x1fu;
    uint32_t man = h & 0x3ffu;
    if (exp == 0x1fu) return sign | 0x7f800000u | (man << 13);   // inf, or a NaN with its payload
    if (exp != 0u) return sign | ((exp + 112u) << 23) | (man << 13);
    if (man == 0u) return sign;
    uint32_t e = 113u;   // man * 2^-24: shift the leading one up to bit 10
    while (!(man & 0x400u)) {
        man <<= 1;
        --e;
    }
    return sign | (e << 23) | ((man & 0x3ffu) << 13);
}

inline uint32_t widen_bits(uint16_t word, int storage) {
    return storage == MI355REC_EMBED_HALF_FP16 ? widen_fp16_bits(word) : static_cast<uint32_t>(word) << 16;
}

inline float widen(uint16_t word, int storage) {
    const uint32_t b = widen_bits(word, storage);
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}

}  // namespace mi355embedhalf
