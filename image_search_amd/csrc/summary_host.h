// summary_host.h — the host-only rules of mi_knn_summarize (summary.hip): the argument check, the integer weight of a
// distance, the per-group slots the device reduces into and how they turn into ids and distances, and the padding of an empty
// table.  The weight and the keys are marked for both sides when a HIP compiler reads this file (summary_kernels.h uses them);
// nothing else in here knows of HIP: tests/cpp/test_summary_host.cpp runs it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/mi355clip.h"
#include "ids.h"

namespace mi {

constexpr uint32_t SUMMARY_MAX_C = 65536;

// MI_OK, or the code with *why set: the handle, then C.  Judged before the handle is followed.
inline int summary_check_args(const void* t, uint32_t C, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (C == 0) { *why = "C must be >= 1"; return MI_ERR_INVALID; }
    if (C > SUMMARY_MAX_C) { *why = "at most 65536 groups"; return MI_ERR_UNSUPPORTED; }
    return MI_OK;
}

// w(d) = floor(min(max(d, 0), 2) * 2^30) for a distance that is not NaN: mi_knn_kmeans_seed's weight (an exact power-of-two
// scaling in fp32, then truncation; w(2) = 2^31 fits)
MI_IDS_HD inline uint32_t summary_weight(float d) {
    const float c = d < 0.0f ? 0.0f : (d > 2.0f ? 2.0f : d);
    return (uint32_t)(c * 1073741824.0f);
}

// the search's 32-bit distance key (knn_shared.h: dist_to_u32 / u32_to_dist) on the host: ascending with the distance, -0 in
// front of +0, every NaN 0xFFFFFFFF
inline uint32_t summary_key_of(float d) {
    uint32_t b;
    std::memcpy(&b, &d, 4);
    if (d != d) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float summary_dist_of(uint32_t k) {
    const uint32_t b = k == 0xFFFFFFFFu ? 0x7FC00000u : ((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
    float d;
    std::memcpy(&d, &b, 4);
    return d;
}

// A group's four 64-bit slots on the device (32 bytes per group), kept as four planes of C words:
//   [0] the smallest (key << 32 | row) over its members (NaN keys included: they sort last); starts as all ones
//   [1] the largest (key << 32 | ~row) over its members whose distance is a number (~row: among equal keys the LOWEST row is
//       the largest word); starts as 0, which no member produces (a key of 0 would be the bits of a negative NaN)
//   [2] measured, [3] spread
constexpr int SUMMARY_PLANES = 4;
constexpr uint64_t SUMMARY_MIN_INIT = 0xFFFFFFFFFFFFFFFFull, SUMMARY_MAX_INIT = 0ull;
MI_IDS_HD inline uint64_t summary_min_word(uint32_t key, uint32_t row) { return ((uint64_t)key << 32) | row; }
MI_IDS_HD inline uint64_t summary_max_word(uint32_t key, uint32_t row) { return ((uint64_t)key << 32) | (uint32_t)~row; }

// slots [4][C] and count [C] -> the caller's arrays (each may be null).  Local rows ascend with their ids (ids.h), so the
// lowest row is the lowest id.
inline void summary_decode(const uint64_t* slots, const uint32_t* count, uint32_t C, const IdMap& map, uint64_t* cover, float* cover_dist,
                           uint64_t* odd, float* odd_dist, uint64_t* measured, uint64_t* spread) {
    for (uint32_t c = 0; c < C; ++c) {
        const uint64_t s[SUMMARY_PLANES] = {slots[c], slots[(size_t)C + c], slots[(size_t)2 * C + c], slots[(size_t)3 * C + c]};
        const bool any = count[c] != 0, num = any && s[2] != 0;
        if (cover) cover[c] = any ? id_of_local(map, (uint32_t)s[0]) : MI_KNN_NO_ID;
        if (cover_dist) cover_dist[c] = any ? summary_dist_of((uint32_t)(s[0] >> 32)) : INFINITY;
        if (odd) odd[c] = num ? id_of_local(map, (uint32_t)~(uint32_t)s[1]) : MI_KNN_NO_ID;
        if (odd_dist) odd_dist[c] = num ? summary_dist_of((uint32_t)(s[1] >> 32)) : INFINITY;
        if (measured) measured[c] = any ? s[2] : 0;
        if (spread) spread[c] = any ? s[3] : 0;
    }
}

// what a table without rows answers: C empty groups
inline void summary_pad(uint32_t C, uint32_t dim, float* centroids, uint64_t* count, uint64_t* cover, float* cover_dist, uint64_t* odd,
                        float* odd_dist, uint64_t* measured, uint64_t* spread, uint64_t* totals) {
    if (centroids) std::memset(centroids, 0, (size_t)C * dim * sizeof(float));
    for (uint32_t c = 0; c < C; ++c) {
        if (count) count[c] = 0;
        if (cover) cover[c] = MI_KNN_NO_ID;
        if (cover_dist) cover_dist[c] = INFINITY;
        if (odd) odd[c] = MI_KNN_NO_ID;
        if (odd_dist) odd_dist[c] = INFINITY;
        if (measured) measured[c] = 0;
        if (spread) spread[c] = 0;
    }
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
}

}  // namespace mi
