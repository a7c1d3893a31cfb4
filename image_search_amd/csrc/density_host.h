// density_host.h — the host-only rules of mi_knn_density, mi_knn_dbscan and mi_index_themes (density.hip): the argument checks,
// the tiles pass 2 visits and skips as the host counts them from the blocks' activity bytes, the dense renumbering of the
// cluster ids (scikit-learn's labels) and the cluster lists in mi_index_duplicates' output shape.  Nothing in here knows of
// HIP: tests/cpp/test_density_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/mi355clip.h"

namespace mi {

// MI_OK, or MI_ERR_INVALID with *why set: the handle, then max_dist (a number >= 0, as for the join).  Judged before the
// handle is followed.
inline int density_check_args(const void* t, float max_dist, const void* counts, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!(max_dist >= 0.0f)) { *why = "max_dist must be a number >= 0"; return MI_ERR_INVALID; }
    if (!counts) { *why = "counts is null"; return MI_ERR_INVALID; }
    return MI_OK;
}
// ... then min_pts >= 1 and the two required outputs (via, via_dist and counts may be null)
inline int dbscan_check_args(const void* t, float max_dist, uint32_t min_pts, const void* cluster, const void* summary, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!(max_dist >= 0.0f)) { *why = "max_dist must be a number >= 0"; return MI_ERR_INVALID; }
    if (min_pts == 0) { *why = "min_pts must be >= 1 (it counts the row itself)"; return MI_ERR_INVALID; }
    if (!cluster || !summary) { *why = "cluster or summary is null"; return MI_ERR_INVALID; }
    return MI_OK;
}

// act[b]: bit 0 = some row of block b has a neighbour within, bit 1 = some row of it is a core.  Tile (bi, bj) is visited iff
// both blocks have bit 0 and one of them bit 1 (pair_tile's SKIP test, pair_kernels.h).
inline bool density_tile_visited(uint8_t fa, uint8_t fb) { return (fa & fb & 1u) && ((fa | fb) & 2u); }

// Prefix counts over the blocks, so that the tiles of a rectangle are counted per tile row, not per tile:
// n1[j] = blocks below j with bit 0, n3[j] = blocks below j with bits 0 and 1.
struct DensityBlocks {
    std::vector<uint8_t> act;
    std::vector<uint32_t> n1, n3;
    void index() {
        n1.assign(act.size() + 1, 0);
        n3.assign(act.size() + 1, 0);
        for (size_t j = 0; j < act.size(); ++j) {
            n1[j + 1] = n1[j] + ((act[j] & 1u) ? 1u : 0u);
            n3[j + 1] = n3[j] + ((act[j] & 3u) == 3u ? 1u : 0u);
        }
    }
    // the tiles on or above the diagonal of rows [r0, r1) x columns [c0, c1): how many the kernel visits and how many it leaves
    void count(uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, uint64_t* visited, uint64_t* skipped) const {
        uint64_t v = 0, all = 0;
        for (uint32_t bi = r0; bi < r1; ++bi) {
            const uint32_t lo = std::max(c0, bi);
            if (lo >= c1) continue;
            all += c1 - lo;
            if (!(act[bi] & 1u)) continue;
            v += (act[bi] & 2u) ? n1[c1] - n1[lo] : n3[c1] - n3[lo];
        }
        *visited = v;
        *skipped = all - v;
    }
};

// cluster [n] (MI_KNN_NO_ID: no cluster) -> labels [n]: 0 .. C - 1 in the order of the cluster ids (a cluster id is the id of the
// cluster's smallest core row), -1 where there is none.  Returns C.
inline uint64_t density_dense_labels(const uint64_t* cluster, uint64_t n, int64_t* labels) {
    std::vector<uint64_t> ids;
    for (uint64_t r = 0; r < n; ++r)
        if (cluster[r] != MI_KNN_NO_ID) ids.push_back(cluster[r]);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    for (uint64_t r = 0; r < n; ++r)
        labels[r] = cluster[r] == MI_KNN_NO_ID ? -1 : (int64_t)(std::lower_bound(ids.begin(), ids.end(), cluster[r]) - ids.begin());
    return ids.size();
}

// The clusters as lists, mi_index_duplicates' shape: gids = the ids of the clustered rows, cluster by cluster, ascending
// inside; the clusters ordered by their smallest MEMBER (which may be a border row below the cluster's id); starts:
// n_clusters + 1 offsets into gids.  ids [n]: the rows' ids.
inline void density_lists(const uint64_t* ids, const uint64_t* cluster, uint64_t n, std::vector<uint64_t>* gids,
                          std::vector<uint64_t>* starts) {
    std::vector<std::pair<uint64_t, uint64_t>> cm;   // (cluster id, member id)
    for (uint64_t r = 0; r < n; ++r)
        if (cluster[r] != MI_KNN_NO_ID) cm.emplace_back(cluster[r], ids[r]);
    std::sort(cm.begin(), cm.end());
    std::vector<std::pair<uint64_t, size_t>> first;   // (smallest member, where the cluster starts in cm)
    for (size_t i = 0; i < cm.size(); ++i)
        if (i == 0 || cm[i].first != cm[i - 1].first) first.emplace_back(cm[i].second, i);
    std::sort(first.begin(), first.end());
    gids->clear();
    starts->clear();
    for (const auto& f : first) {
        starts->push_back(gids->size());
        for (size_t i = f.second; i < cm.size() && cm[i].first == cm[f.second].first; ++i) gids->push_back(cm[i].second);
    }
    starts->push_back(gids->size());
}

}  // namespace mi
