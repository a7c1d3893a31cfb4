// density_call.h — stage 1 of the density passes, once, for the three units that run them: density.hip, density_levels.hip
// (one table: the tiles on or above the diagonal) and density_sharded.hip (a shard with itself, or with a column chunk of
// another shard: every tile of the rectangle).  A unit keeps its own stage 2 and what surrounds the passes.
#pragma once
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "density_sharded_host.h"     // DensityBlocks, CrossBlocks: the tiles pass 2 visits, counted on the host
#include "density_sharded_kernels.h"  // the four tile kernels (templates only: nothing is compiled that a unit does not launch)
#include "join_between_host.h"        // tile_strips: the walk every pass makes over its tiles
#include "two_stage.h"

namespace mi {

// one side of the tiles as stage 1 sees it: n rows; act: the blocks' activity bytes on the device (pass 2)
struct DensitySide {
    const uint16_t* mirror;
    const float* xx;
    const uint64_t* tomb;
    uint32_t n;
    const uint8_t* act;
};

// SELF: the rows of `a` against themselves (b is not read); else the rows of a against the column chunk b.
template <bool SELF>
struct DensityStage1 {
    hipStream_t s;
    DensitySide a, b;
    const DensityBlocks* blocks;   // a's activity bytes on the host, indexed (pass 2)
    const CrossBlocks* cross;      // !SELF: the prefix counts of b's (pass 2)
    float c;                       // 1 - (max_dist + eps2)
    uint32_t cand_cap;
    uint2* d_cand;
    unsigned long long* d_count;   // the word the launch in flight counts its candidates in
    uint64_t* stats;               // [8] of mi_knn_dbscan_stats: [2] tiles of pass 1, [4] / [5] visited / skipped in pass 2, [7] launches

    // Stage 1 of pass PASS for rect_stages (two_stage.h).  SELF: bc0 is raised to the diagonal, the tiles are the triangle's.
    // rect_stages hands a candidate buffer to stage 2 only when the launch that filled it fitted, and redoes the ground of
    // one that did not in halves without consuming anything: every pair reaches stage 2 exactly once, also across overflow
    // halvings (degrees, which are adds, rely on that; unions and minima would not mind a repeat).  The tile counts follow
    // the same rule: only a launch whose candidates were consumed counts its tiles, so visited + skipped is the ground.
    template <int NCH, int PASS>
    unsigned long long stage1(uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) {
        if (SELF) c0 = std::max(c0, r0);
        if (c0 >= c1) return 0;
        uint64_t visited = 0, skipped = 0;
        if (PASS == 2) {
            if (SELF) blocks->count(r0, r1, c0, c1, &visited, &skipped);
            else cross->count(blocks->act.data(), r0, r1, c0, c1, &visited, &skipped);
            if (visited == 0) { stats[5] += skipped; return 0; }   // every workgroup would leave at once
        } else if (SELF) {
            for (uint32_t bi = r0; bi < r1; ++bi) visited += c1 - std::max(c0, bi);
        } else {
            visited = (uint64_t)(r1 - r0) * (c1 - c0);
        }
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
        const dim3 grid(c1 - c0, r1 - r0);
        // One per NCH, PASS and SELF, i.e. one per kernel, and ONE for the three units that include this header: the object and
        // the kernel's host stub are both merged across the units of the library, which is intended (assign_call.h does the same).
        static DevOnce once;
        if constexpr (SELF && PASS == 1) {
            allow_lds_once(once, join_tiles_kernel<NCH>, JOIN_LDS);
            hipLaunchKernelGGL((join_tiles_kernel<NCH>), grid, dim3(256), JOIN_LDS, s, a.mirror, a.xx, a.tomb, a.n, 0u, r0, c0, c, cand_cap,
                               d_cand, d_count);
        } else if constexpr (SELF) {
            allow_lds_once(once, density_tiles_kernel<NCH>, JOIN_LDS);
            hipLaunchKernelGGL((density_tiles_kernel<NCH>), grid, dim3(256), JOIN_LDS, s, a.mirror, a.xx, a.tomb, a.act, a.n, r0, c0, c,
                               cand_cap, d_cand, d_count);
        } else if constexpr (PASS == 1) {
            allow_lds_once(once, cross_tiles_kernel<NCH>, JOIN_LDS);
            hipLaunchKernelGGL((cross_tiles_kernel<NCH>), grid, dim3(256), JOIN_LDS, s, a.mirror, a.xx, a.tomb, a.n, b.mirror, b.xx, b.tomb,
                               b.n, 0u, 0u, r0, c0, c, cand_cap, d_cand, d_count);
        } else {
            allow_lds_once(once, density_cross_tiles_kernel<NCH>, JOIN_LDS);
            hipLaunchKernelGGL((density_cross_tiles_kernel<NCH>), grid, dim3(256), JOIN_LDS, s, a.mirror, a.xx, a.tomb, a.act, a.n, b.mirror,
                               b.xx, b.tomb, b.act, b.n, r0, c0, c, cand_cap, d_cand, d_count);
        }
        HIP_CHECK(hipGetLastError());
        ++stats[7];
        const unsigned long long n = read_count(d_count, s);
        if (n <= cand_cap) {
            if (PASS == 1) stats[2] += visited;
            else { stats[4] += visited; stats[5] += skipped; }
        }
        return n;
    }
};

}  // namespace mi
