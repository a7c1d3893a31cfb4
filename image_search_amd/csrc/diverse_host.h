// diverse_host.h — the host-only pieces of mi_knn_search_diverse (diverse.hip): the argument rules, the layout of the one
// record the device writes and the host copies back, and how that record (or "nothing in the pool") reaches the caller's
// arrays, some of which may be NULL.  No HIP in here: tests/cpp/test_diverse_host.cpp runs it under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../include/mi355clip.h"

namespace mi {

constexpr uint32_t DIVERSE_MAX_POOL = 4096;

// MI_OK, or the error the contract names with *why set.  Zero / null: MI_ERR_INVALID before any MI_ERR_UNSUPPORTED.
inline int diverse_check_args(const void* t, const void* q, uint32_t k, uint32_t pool, float min_gap, const void* among, uint64_t n_among,
                              const void* idx, const void* dist, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!q || !idx || !dist) { *why = "null query/result pointer"; return MI_ERR_INVALID; }
    if (k == 0 || pool == 0) { *why = "k and pool must be >= 1"; return MI_ERR_INVALID; }
    if (!(min_gap >= 0.0f)) { *why = "min_gap must be a number >= 0"; return MI_ERR_INVALID; }
    if (!among && n_among != 0) { *why = "among is null"; return MI_ERR_INVALID; }
    if (pool > DIVERSE_MAX_POOL) { *why = "pool must be <= 4096"; return MI_ERR_UNSUPPORTED; }
    if (k > pool) { *why = "k must be <= pool"; return MI_ERR_UNSUPPORTED; }
    return MI_OK;
}

// The record: idx [k] u64 | dist [k] f32 | hidden [k] u32 | rep [pool] u32 | state [4] u32 = {n_kept, pool entries hidden,
// conflicting pairs, P}.  Offsets in bytes; every array starts on a multiple of its element size (idx first, then 4-byte
// arrays only).
struct DiverseRecord {
    size_t idx, dist, hidden, rep, state, bytes;
};
inline DiverseRecord diverse_record(uint32_t k, uint32_t pool) {
    DiverseRecord r;
    r.idx = 0;
    r.dist = (size_t)k * sizeof(uint64_t);
    r.hidden = r.dist + (size_t)k * sizeof(float);
    r.rep = r.hidden + (size_t)k * sizeof(uint32_t);
    r.state = r.rep + (size_t)pool * sizeof(uint32_t);
    r.bytes = r.state + 4 * sizeof(uint32_t);
    return r;
}

// the record as the device left it -> the caller's arrays (hidden, rep, n_kept may be NULL); returns the state words
inline void diverse_unpack(const unsigned char* rec, uint32_t k, uint32_t pool, uint64_t* idx, float* dist, uint32_t* hidden, uint32_t* rep,
                           uint32_t* n_kept, uint32_t state[4]) {
    const DiverseRecord r = diverse_record(k, pool);
    std::memcpy(state, rec + r.state, 4 * sizeof(uint32_t));
    std::memcpy(idx, rec + r.idx, (size_t)k * sizeof(uint64_t));
    std::memcpy(dist, rec + r.dist, (size_t)k * sizeof(float));
    if (hidden) std::memcpy(hidden, rec + r.hidden, (size_t)k * sizeof(uint32_t));
    if (rep) std::memcpy(rep, rec + r.rep, (size_t)pool * sizeof(uint32_t));
    if (n_kept) *n_kept = state[0];
}

// an empty pool: all padding
inline void diverse_pad(uint32_t k, uint32_t pool, uint64_t* idx, float* dist, uint32_t* hidden, uint32_t* rep, uint32_t* n_kept) {
    for (uint32_t j = 0; j < k; ++j) {
        idx[j] = MI_KNN_NO_ID;
        dist[j] = std::numeric_limits<float>::infinity();
        if (hidden) hidden[j] = 0;
    }
    if (rep)
        for (uint32_t r = 0; r < pool; ++r) rep[r] = MI_KNN_NO_LABEL;
    if (n_kept) *n_kept = 0;
}

}  // namespace mi
