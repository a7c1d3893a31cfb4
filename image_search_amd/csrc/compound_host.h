// compound_host.h — the host-only pieces of mi_knn_search_compound (compound.hip): the argument rules, the term set as the
// scan wants it (padded to 2 / 4 / 8 resident terms with their roles and thresholds), the per-CU factor of "compound_blocks",
// the layout of the one record the device writes, and how it (or "no candidate") reaches the caller's arrays.  No HIP in
// here: tests/cpp/test_compound_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mi355clip.h"

namespace mi {

constexpr uint32_t COMPOUND_TERMS_MAX = 8, COMPOUND_K_MAX = 4096;

// MI_OK, or the error the contract names with *why set.  Zero / null / unknown mode first (MI_ERR_INVALID), then the limits
// (MI_ERR_UNSUPPORTED), then the thresholds (MI_ERR_INVALID), which are read only once their count is known to be small.
inline int compound_check_args(const void* t, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within,
                               uint32_t n_neg, uint32_t k, const void* among, uint64_t n_among, const void* idx, const void* dist,
                               const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!pos || !idx || !dist) { *why = "null term/result pointer"; return MI_ERR_INVALID; }
    if (n_pos == 0 || k == 0) { *why = "n_pos and k must be >= 1"; return MI_ERR_INVALID; }
    if (mode != MI_COMPOUND_ALL && mode != MI_COMPOUND_ANY) { *why = "mode must be MI_COMPOUND_ALL or MI_COMPOUND_ANY"; return MI_ERR_INVALID; }
    if (n_neg && (!neg || !neg_within)) { *why = "negative terms without neg / neg_within"; return MI_ERR_INVALID; }
    if (!among && n_among != 0) { *why = "among is null"; return MI_ERR_INVALID; }
    if (n_pos > COMPOUND_TERMS_MAX || n_neg > COMPOUND_TERMS_MAX || n_pos + n_neg > COMPOUND_TERMS_MAX) {
        *why = "n_pos + n_neg must be <= 8"; return MI_ERR_UNSUPPORTED;
    }
    if (k > COMPOUND_K_MAX) { *why = "k must be <= 4096"; return MI_ERR_UNSUPPORTED; }
    for (uint32_t j = 0; j < n_neg; ++j)
        if (!(neg_within[j] >= 0.0f)) { *why = "neg_within must be numbers >= 0"; return MI_ERR_INVALID; }
    return MI_OK;
}

// The resident term set: the T = n_pos + n_neg terms, positives first, then copies of the first positive term up to 2 / 4 / 8
// (a repeated positive term changes no maximum and no minimum).  neg_mask bit u = term u is negative; within[u] its threshold.
struct CompoundSet {
    uint32_t T = 0, padded = 0, neg_mask = 0;
    float within[COMPOUND_TERMS_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<float> terms;   // [padded][dim]
};
inline uint32_t compound_padded(uint32_t T) { return T <= 2 ? 2u : T <= 4 ? 4u : 8u; }
inline CompoundSet compound_set(const float* pos, uint32_t n_pos, const float* neg, const float* neg_within, uint32_t n_neg, uint32_t dim) {
    CompoundSet c;
    c.T = n_pos + n_neg;
    c.padded = compound_padded(c.T);
    c.terms.resize((size_t)c.padded * dim);
    std::memcpy(c.terms.data(), pos, (size_t)n_pos * dim * sizeof(float));
    if (n_neg) std::memcpy(c.terms.data() + (size_t)n_pos * dim, neg, (size_t)n_neg * dim * sizeof(float));
    for (uint32_t u = c.T; u < c.padded; ++u) std::memcpy(c.terms.data() + (size_t)u * dim, pos, (size_t)dim * sizeof(float));
    for (uint32_t j = 0; j < n_neg; ++j) {
        c.neg_mask |= 1u << (n_pos + j);
        c.within[n_pos + j] = neg_within[j];
    }
    return c;
}

// the scan's workgroups with "compound_blocks" = 0: the batched search's grid, two per CU (scan_grid of scan_call.h)
constexpr uint32_t COMPOUND_BLOCKS_PER_CU = 2;

// The record: idx [k] u64 | stats [4] u64 = {excluded, NaN scores, -, results written} | dist [k] f32 | term_dist [k][T] f32
struct CompoundRecord {
    size_t idx, stats, dist, term_dist, bytes;
};
inline CompoundRecord compound_record(uint32_t k, uint32_t T) {
    CompoundRecord r;
    r.idx = 0;
    r.stats = (size_t)k * sizeof(uint64_t);
    r.dist = r.stats + 4 * sizeof(uint64_t);
    r.term_dist = r.dist + (size_t)k * sizeof(float);
    r.bytes = r.term_dist + (size_t)k * T * sizeof(float);
    return r;
}
inline void compound_unpack(const unsigned char* rec, uint32_t k, uint32_t T, uint64_t* idx, float* dist, float* term_dist, uint64_t stats[4]) {
    const CompoundRecord r = compound_record(k, T);
    std::memcpy(stats, rec + r.stats, 4 * sizeof(uint64_t));
    std::memcpy(idx, rec + r.idx, (size_t)k * sizeof(uint64_t));
    std::memcpy(dist, rec + r.dist, (size_t)k * sizeof(float));
    if (term_dist) std::memcpy(term_dist, rec + r.term_dist, (size_t)k * T * sizeof(float));
}

// no candidate at all: all padding
inline void compound_pad(uint32_t k, uint32_t T, uint64_t* idx, float* dist, float* term_dist) {
    for (uint32_t j = 0; j < k; ++j) {
        idx[j] = MI_KNN_NO_ID;
        dist[j] = std::numeric_limits<float>::infinity();
    }
    if (term_dist)
        for (size_t j = 0; j < (size_t)k * T; ++j) term_dist[j] = std::numeric_limits<float>::infinity();
}

}  // namespace mi
