// density_sharded_host.h — the host-only rules of mi_knn_sharded_density and mi_knn_sharded_dbscan (density_sharded.hip): the
// argument checks (the single table's, density_host.h) and the row limit, the tiles a cross rectangle of pass 2 visits and
// skips as the host counts them from two arrays of activity bytes, the scatter of a shard's local arrays to global rows, and
// a plain forest merge that restates what density_forest_merge_kernel computes.  Nothing in here knows of HIP:
// tests/cpp/test_density_sharded_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mi355clip.h"
#include "density_host.h"
#include "ids.h"

namespace mi {

// ---- the row limit (the argument rules are density_check_args and dbscan_check_args of density_host.h) ------------------------
// a forest entry and the low half of a border key hold a global row
inline bool sharded_density_rows_ok(uint64_t rows) { return rows < (1ull << 32); }

// ---- the tiles of a cross rectangle ---------------------------------------------------------------------------------------
// Rows: the blocks of the row-side shard; columns: the blocks of one column chunk.  Tile (bi, bj) is visited iff
// density_tile_visited(row[bi], col[bj]) (density_cross_tiles_kernel's test); there is no diagonal.  Prefix counts over the
// chunk's blocks, as DensityBlocks keeps them: n1[j] = blocks below j with bit 0, n3[j] = ... with bits 0 and 1.
struct CrossBlocks {
    std::vector<uint32_t> n1, n3;
    void index(const uint8_t* col, size_t n) {
        n1.assign(n + 1, 0);
        n3.assign(n + 1, 0);
        for (size_t j = 0; j < n; ++j) {
            n1[j + 1] = n1[j] + ((col[j] & 1u) ? 1u : 0u);
            n3[j + 1] = n3[j] + ((col[j] & 3u) == 3u ? 1u : 0u);
        }
    }
    // the tiles of row blocks [r0, r1) x column blocks [c0, c1) of the chunk
    void count(const uint8_t* row, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, uint64_t* visited, uint64_t* skipped) const {
        uint64_t v = 0;
        for (uint32_t bi = r0; bi < r1; ++bi) {
            if (!(row[bi] & 1u)) continue;
            v += (row[bi] & 2u) ? n1[c1] - n1[c0] : n3[c1] - n3[c0];
        }
        *visited = v;
        *skipped = (uint64_t)(r1 - r0) * (c1 - c0) - v;
    }
};

// ---- local rows -> global rows ----------------------------------------------------------------------------------------------
// out[id_of_local(map, r)] = local[r] for the n local rows of one shard (a shard of a sharded table has base 0: its ids are
// the table's global rows)
template <class T>
inline void scatter_to_global(const IdMap& map, const T* local, uint64_t n, T* out) {
    for (uint64_t r = 0; r < n; ++r) out[id_of_local(map, r)] = local[r];
}

// ---- the forest merge, restated ---------------------------------------------------------------------------------------------
// Forests over the same G rows with parent[x] <= x, equality exactly at a root.  After the call `into` holds the union of
// both: two rows share a root iff a chain of links of either forest joins them, and the root of a component is its smallest row.
inline uint32_t forest_find(std::vector<uint32_t>& parent, uint32_t x) {
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}
inline uint64_t forest_merge(std::vector<uint32_t>& into, const std::vector<uint32_t>& other) {
    uint64_t merged = 0;
    for (uint32_t g = 0; g < (uint32_t)other.size(); ++g) {
        if (other[g] == g) continue;
        const uint32_t a = forest_find(into, g), b = forest_find(into, other[g]);
        if (a == b) continue;
        into[std::max(a, b)] = std::min(a, b);
        ++merged;
    }
    return merged;
}

}  // namespace mi
