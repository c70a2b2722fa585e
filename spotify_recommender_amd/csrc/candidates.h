// candidates.h — CANDIDATE LISTS (include/mi355rec_diag.h, "CANDIDATE LISTS"): a request's list of global row ids, on the host.  The
// list's checks, its reduction to the SORTED, DISTINCT LOCAL ROWS of one shard as uint32 (what playlist_scan_kernel's gather branch
// reads: csrc/playlist.hip.h, "CANDIDATE LISTS"), the split of a node handle's list over its shards' ranges and the membership test
// of the CPU backend, shared by the single handle (engine_playlist.hip.h), the node handle (sharded.hip) and the CPU backend.
// Host only: no HIP type or call (tests/candidates_check.cpp compiles it with g++).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mi355cand {

// True when the list's count cannot be used: n < 0, a null list with n > 0, n > max_n (MI355REC_MAX_CANDIDATES); msg[0..cap) says why.
// No id is read: the single handle checks the ids in the pass that reduces them (reduce, below).
inline bool invalid_count(const int64_t* ids, int64_t n, int64_t max_n, char* msg, size_t cap) {
    if (n < 0) {
        std::snprintf(msg, cap, "candidate list: n_candidates must not be negative, got %lld", static_cast<long long>(n));
        return true;
    }
    if (n > 0 && !ids) {
        std::snprintf(msg, cap, "candidate list: null list with n_candidates %lld", static_cast<long long>(n));
        return true;
    }
    if (n > max_n) {
        std::snprintf(msg, cap, "candidate list: n_candidates %lld above MI355REC_MAX_CANDIDATES (%lld)", static_cast<long long>(n),
                      static_cast<long long>(max_n));
        return true;
    }
    return false;
}

// The message for an id outside [0, id_end).  (id_end: 2^32 on a single handle, as for row sets; the rows of a node handle.)
inline void bad_id_message(int64_t id, int64_t id_end, char* msg, size_t cap) {
    std::snprintf(msg, cap, "candidate list: id %lld out of [0, %lld)", static_cast<long long>(id), static_cast<long long>(id_end));
}

// invalid_count, then every id in [0, id_end) in a pass of its own: the node handle, which knows its catalogue's rows before any
// shard sees the list.  msg names the first id that is not.
inline bool invalid_list(const int64_t* ids, int64_t n, int64_t max_n, int64_t id_end, char* msg, size_t cap) {
    if (invalid_count(ids, n, max_n, msg, cap)) return true;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= id_end) {
            bad_id_message(ids[i], id_end, msg, cap);
            return true;
        }
    return false;
}

struct Reduced {
    int64_t count = 0;      // distinct ids of [lo, hi) in the list: the entries of out[]
    bool ascending = true;  // the in-range ids came strictly ascending: nothing was sorted
    int64_t bad = -1;       // (id_end >= 0 only) the index of the first id outside [0, id_end): out[] is then of no use
};

// The checked list reduced to the rows of the shard [lo, hi): out[0..count) = id - lo, strictly ascending (hi - lo <= 2^32, so a local
// row fits uint32).  out holds n entries.  One pass keeps the in-range ids and tests whether they already ascend strictly (the
// output of a first stage that walks an index usually does); only otherwise are they sorted and made distinct.
// id_end >= 0: the same pass checks every id against [0, id_end) and stops at the first that is not (Reduced::bad), so a list is
// read once where its ids have not been checked yet; id_end < 0: they have been.  (0 <= lo <= hi <= id_end where it is given.)
inline Reduced reduce(const int64_t* ids, int64_t n, int64_t lo, int64_t hi, uint32_t* out, int64_t id_end = -1) {
    Reduced r;
    int64_t prev = -1;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        if (id < lo || id >= hi) {
            if (id_end >= 0 && (id < 0 || id >= id_end)) {
                r.bad = i;
                return r;
            }
            continue;
        }
        const int64_t row = id - lo;
        r.ascending = r.ascending && row > prev;
        prev = row;
        out[r.count++] = static_cast<uint32_t>(row);
    }
    if (!r.ascending) {
        std::sort(out, out + r.count);
        r.count = static_cast<int64_t>(std::unique(out, out + r.count) - out);
    }
    return r;
}

// CANDIDATE SCORES: from list order to the reduced list.  rows[0..red.count) and `red` are what reduce made of the same ids, lo and hi;
// pos holds n entries: pos[i] = the index of ids[i] - lo in rows, or -1 when ids[i] is outside [lo, hi).  One pass when the list
// came strictly ascending (the in-range ids ARE the reduced list, in order), a binary search per id otherwise.
inline void positions(const int64_t* ids, int64_t n, int64_t lo, int64_t hi, const uint32_t* rows, const Reduced& red, int64_t* pos) {
    int64_t next = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        if (id < lo || id >= hi) pos[i] = -1;
        else if (red.ascending) pos[i] = next++;
        else pos[i] = std::lower_bound(rows, rows + red.count, static_cast<uint32_t>(id - lo)) - rows;   // (found: reduce kept it)
    }
}

// A node handle's checked list for the shard [lo, hi): the ids of that range, global, in list order (duplicates stay: the shard's
// own reduce drops them).  out is cleared first.
inline void split(const int64_t* ids, int64_t n, int64_t lo, int64_t hi, std::vector<int64_t>* out) {
    out->clear();
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= lo && ids[i] < hi) out->push_back(ids[i]);
}

// Is `row` among the reduced rows (ascending)?  What the CPU backend asks per row.
inline bool contains(const uint32_t* rows, int64_t count, int64_t row) {
    return row >= 0 && row <= static_cast<int64_t>(UINT32_MAX) && std::binary_search(rows, rows + count, static_cast<uint32_t>(row));
}

}  // namespace mi355cand
