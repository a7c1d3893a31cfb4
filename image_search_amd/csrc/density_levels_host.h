// density_levels_host.h — the host-only rules of mi_knn_density_levels, mi_knn_dbscan_levels and mi_dbscan_levels_tree
// (density_levels.hip): the argument checks, the thresholds as the kernels take them (by value) and the tree between the
// levels.  Nothing in here knows of HIP: tests/cpp/test_density_levels_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/mi355clip.h"

namespace mi {

// the thresholds of a call, ascending; d[n ..] repeat the top one (never read: every loop over the levels stops at n)
struct DensityLevels {
    float d[MI_KNN_LEVELS_MAX];
    uint32_t n;
};

// MI_OK, or MI_ERR_INVALID with *why set: 1 <= n_levels <= MI_KNN_LEVELS_MAX, every entry a number >= 0, strictly ascending
inline int density_levels_check(const float* max_dists, uint32_t n_levels, const char** why) {
    *why = "";
    if (!max_dists) { *why = "max_dists is null"; return MI_ERR_INVALID; }
    if (n_levels == 0 || n_levels > MI_KNN_LEVELS_MAX) { *why = "n_levels must be 1 .. MI_KNN_LEVELS_MAX"; return MI_ERR_INVALID; }
    for (uint32_t l = 0; l < n_levels; ++l) {
        if (!(max_dists[l] >= 0.0f)) { *why = "every entry of max_dists must be a number >= 0"; return MI_ERR_INVALID; }
        if (l > 0 && !(max_dists[l - 1] < max_dists[l])) { *why = "max_dists must be strictly ascending"; return MI_ERR_INVALID; }
    }
    return MI_OK;
}
// the handle first, judged before it is followed (density_check_args' order), then the levels, then the outputs
inline int density_levels_check_args(const void* t, const float* max_dists, uint32_t n_levels, const void* counts, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    const int bad = density_levels_check(max_dists, n_levels, why);
    if (bad != MI_OK) return bad;
    if (!counts) { *why = "counts is null"; return MI_ERR_INVALID; }
    return MI_OK;
}
inline int dbscan_levels_check_args(const void* t, const float* max_dists, uint32_t n_levels, uint32_t min_pts, const void* cluster,
                                    const void* summary, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    const int bad = density_levels_check(max_dists, n_levels, why);
    if (bad != MI_OK) return bad;
    if (min_pts == 0) { *why = "min_pts must be >= 1 (it counts the row itself)"; return MI_ERR_INVALID; }
    if (!cluster || !summary) { *why = "cluster or summary is null"; return MI_ERR_INVALID; }
    return MI_OK;
}

// max_dists has passed density_levels_check
inline DensityLevels density_levels_make(const float* max_dists, uint32_t n_levels) {
    DensityLevels lv;
    lv.n = n_levels;
    for (uint32_t l = 0; l < MI_KNN_LEVELS_MAX; ++l) lv.d[l] = max_dists[std::min(l, n_levels - 1)];
    return lv;
}

// The first level dist lies within, n if none (a NaN compares false everywhere: in no level).  The thresholds ascend, so the
// levels that fail `dist <= d[l]` — the single call's compare — are a prefix, and counting them names the first that holds.
// The kernels (density_levels_kernels.h) make the same count.
inline uint32_t density_level_of_host(const DensityLevels& lv, float dist) {
    uint32_t l = 0;
    for (uint32_t j = 0; j < lv.n; ++j) l += !(dist <= lv.d[j]) ? 1u : 0u;
    return l;
}

struct LevelEdge {
    uint32_t level;
    uint64_t child, parent;
};

// mi_dbscan_levels_tree behind its null checks.  cluster, counts: [n_levels][rows].  MI_OK and *edges ascending by
// (level, child), or MI_ERR_INVALID with *why set and *edges untouched.
inline int dbscan_levels_tree(const uint64_t* cluster, const uint32_t* counts, uint64_t rows, uint32_t n_levels, uint32_t min_pts,
                              std::vector<LevelEdge>* edges, const char** why) {
    *why = "";
    if (n_levels == 0 || n_levels > MI_KNN_LEVELS_MAX) { *why = "n_levels must be 1 .. MI_KNN_LEVELS_MAX"; return MI_ERR_INVALID; }
    if (min_pts == 0) { *why = "min_pts must be >= 1 (it counts the row itself)"; return MI_ERR_INVALID; }
    std::vector<LevelEdge> out;
    std::vector<std::pair<uint64_t, uint64_t>> cp;   // (child, parent) per core row of one level
    for (uint32_t l = 0; l + 1 < n_levels; ++l) {
        const uint64_t* lo = cluster + (size_t)l * rows;
        const uint64_t* hi = lo + rows;
        const uint32_t* deg = counts + (size_t)l * rows;
        cp.clear();
        for (uint64_t r = 0; r < rows; ++r) {
            if (lo[r] == MI_KNN_NO_ID || (uint64_t)deg[r] + 1 < min_pts) continue;
            if (hi[r] == MI_KNN_NO_ID) { *why = "a core row of one level is in no cluster of the next"; return MI_ERR_INVALID; }
            cp.emplace_back(lo[r], hi[r]);
        }
        std::sort(cp.begin(), cp.end());
        for (size_t i = 0; i < cp.size(); ++i) {
            if (i > 0 && cp[i].first == cp[i - 1].first) {
                if (cp[i].second != cp[i - 1].second) { *why = "the core rows of one cluster lie in two clusters of the next level"; return MI_ERR_INVALID; }
                continue;
            }
            out.push_back(LevelEdge{l, cp[i].first, cp[i].second});
        }
    }
    edges->swap(out);
    return MI_OK;
}

}  // namespace mi
