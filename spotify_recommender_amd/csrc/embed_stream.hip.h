// embed_stream.hip.h — the kernels of libmi355rec_embed_stream.so (gfx950 only; include/mi355rec_embed_stream.h).
//
// The scans are the other embedding libraries' bodies, instantiated here: embed_stream_scan_kernel<Rows, kDimT> is one
// call of embed_scan_body (embed.hip.h) over EmbedRowsF32 or EmbedRowsHalf<storage> (embed_half.hip.h), the user batches
// run embed_batch_scan_kernel<kDimT, 8> (embed_batch.hip.h), and merge_kernel (merge.hip.h) serves as it is.  What is NEW
// are the two small kernels that replace the host on either side of them, one workgroup per user, neither on the
// bandwidth-critical path:
//
// embed_stream_prepare_kernel turns a user's L <= 1024 global int64 ids into the list the scans search: thread t maps id t
// to its local row, or to kNoRow = 0xFFFFFFFF when the id is negative or outside [row_base, row_base + n); threads from L
// on hold kNoRow; the workgroup (the next power of two from L on, at least one wave) sorts ascending with a bitonic
// network, one element per thread in a register; the first L words are stored.  Duplicates stay and kNoRow sorts behind
// every row: both scan bodies search with a lower bound and compare for equality (embed.hip.h, `pass = !(lo < n_exclude &&
// s_excl[lo] == local)`; embed_batch.hip.h, `pass = !(lo < ex_n[i] && list[lo] == local)`), so a repeated row is found at
// its first copy and kNoRow, which no row equals, is never found — n_exclude = L as given.
//   The exchange: a step at distance j < 64 stays inside the wave (__shfl_xor, no LDS); a step at j >= 64 goes through
// LDS, thread t stores word t and loads word t ^ j — 64 consecutive words per wave instruction either way (t ^ j keeps the
// lane bits), so no two lanes of an instruction meet on a bank.
//
// embed_stream_finish_kernel turns a user's merged keys [eff] (sorted descending, 0 behind the last) into out_idx /
// out_score [topn] and out_count as mi355embed::write_result does on the host: count = the non-zero keys, id = ~low word,
// score = the ordered image's float, -1 / 0 from count to topn.
#pragma once

#include "embed_batch.hip.h"
#include "embed_half.hip.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int kEmbedStreamMaxExclude = 1024;   // MI355REC_EMBED_STREAM_MAX_EXCLUDE: the widest prepare workgroup
constexpr int kEmbedStreamFinishBlock = 256;
constexpr uint32_t kEmbedStreamNoRow = 0xFFFFFFFFu;

// The single-user scan over either layout of rows: embed_scan_body's arguments and both of its forms.
template <class Rows, int kDimT>
__global__ __launch_bounds__(kEmbedBlock, 4) void embed_stream_scan_kernel(
    const typename Rows::Word* __restrict__ table, int64_t n, int64_t row_base, const float* __restrict__ user, const float* __restrict__ audio_s,
    const uint32_t* __restrict__ exclude, EmbedArgs a, uint64_t* __restrict__ block_lists, float* __restrict__ out_v, float* __restrict__ out_c) {
    embed_scan_body<Rows, kDimT>(table, n, row_base, user, audio_s, exclude, a, block_lists, out_v, out_c);
}

// ids: gridDim.x x L global ids (user b's row is ids + b * L; L >= 1); blockDim.x: the next power of two from L on, at
// least 64.  rows_out: gridDim.x x L sorted local rows; offsets_out: null, or gridDim.x + 1 offsets b * L.
__global__ __launch_bounds__(kEmbedStreamMaxExclude) void embed_stream_prepare_kernel(
    const int64_t* __restrict__ ids, int L, int64_t row_base, int64_t n, uint32_t* __restrict__ rows_out, int64_t* __restrict__ offsets_out) {
    __shared__ uint32_t s_word[kEmbedStreamMaxExclude];
    const int t = threadIdx.x;
    const int width = blockDim.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * L;

    uint32_t v = kEmbedStreamNoRow;
    if (t < L) {
        const int64_t id = ids[first + t];
        if (id >= 0 && id >= row_base && id - row_base < n) v = static_cast<uint32_t>(id - row_base);   // (compared before the subtraction)
    }
    for (int k = 2; k <= width; k <<= 1) {        // uniform
        for (int j = k >> 1; j > 0; j >>= 1) {   // uniform
            uint32_t other;
            if (j >= 64) {
                s_word[t] = v;
                __syncthreads();
                other = s_word[t ^ j];
                __syncthreads();   // (every thread has read before the next step stores)
            } else {
                other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), j, 64));
            }
            const bool keep_min = ((t & k) == 0) == ((t & j) == 0);
            const uint32_t lo = v < other ? v : other;
            const uint32_t hi = v < other ? other : v;
            v = keep_min ? lo : hi;
        }
    }
    if (t < L) rows_out[first + t] = v;
    if (offsets_out && t == 0) {
        offsets_out[blockIdx.x] = first;
        if (blockIdx.x == gridDim.x - 1) offsets_out[gridDim.x] = first + L;
    }
}

// keys: gridDim.x x eff merged keys (eff >= 0); out_idx / out_score: gridDim.x x topn; out_count: gridDim.x.  out_score and
// out_count may be null.
__global__ __launch_bounds__(kEmbedStreamFinishBlock) void embed_stream_finish_kernel(
    const uint64_t* __restrict__ keys, int eff, int topn, int64_t* __restrict__ out_idx, float* __restrict__ out_score, int32_t* __restrict__ out_count) {
    __shared__ int s_count;
    const int t = threadIdx.x;
    const uint64_t* const mine = keys + static_cast<int64_t>(blockIdx.x) * eff;
    if (t == 0) s_count = 0;
    __syncthreads();
    for (int base = 0; base < eff; base += kEmbedStreamFinishBlock) {   // uniform
        const int i = base + t;
        const uint64_t there = __ballot(i < eff && mine[i] != 0ull);
        if ((t & 63) == 0 && there) atomicAdd(&s_count, __popcll(there));
    }
    __syncthreads();
    const int count = s_count;
    const int64_t out0 = static_cast<int64_t>(blockIdx.x) * topn;
    for (int i = t; i < topn; i += kEmbedStreamFinishBlock) {
        const bool have = i < count;
        const uint64_t key = have ? mine[i] : 0ull;
        out_idx[out0 + i] = have ? static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(key))) : static_cast<int64_t>(-1);
        if (out_score) out_score[out0 + i] = have ? ordered_to_score(static_cast<uint32_t>(key >> 32)) : 0.0f;
    }
    if (out_count && t == 0) out_count[blockIdx.x] = count;
}

}  // namespace mi355
