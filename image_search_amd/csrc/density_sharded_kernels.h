// density_sharded_kernels.h — device code of mi_knn_sharded_density and mi_knn_sharded_dbscan (density_sharded.hip): the
// passes of density_kernels.h over the pairs W of a block-cyclic table, those that cross shards included.
//
// No kernel follows a pointer into another device's memory and there are no atomics across devices.  A piece of work is a
// shard with itself or a row-side shard A with a column chunk of shard B; it runs on A's device and sees B through pointers
// that are valid there: B's own arrays when B lives on that device, or chunk-local copies the host moves and merges between
// launches.  What is merged is an integer sum (degrees), a 64-bit minimum (border keys) or a union (forests): all three give
// the same result in any order, so the result does not depend on shard count, chunking or arrival order.
//
// Pass 1.  Stage 1 is cross_tiles_kernel (join_between_kernels.h) as it stands; stage 2, density_count_between_kernel, is
// cross_rescore_kernel's distance (pair_dist, pair_kernels.h) under its rule "the row with the smaller id is the query", the compaction replaced by
// deg_a[ra] += 1, deg_col[cb] += 1.
//
// Pass 2.  Stage 1, density_cross_tiles_kernel, is cross_tiles_kernel behind the activity test of density_tiles_kernel
// (pair_tile's SKIP), the row block's byte and the column block's byte taken from two arrays.  Stage 2 of every piece, a shard's self piece
// included, is density_link_between_kernel: the forest it unites in spans the GLOBAL rows of the whole table (one forest per
// shard, on its device), a border key names the core by its global row.
//
// Behind the passes (the small plain kernels of density_sharded.hip, kept out of this header so that the single-table units,
// which include it for the tile kernels, do not compile them): density_forest_merge_kernel unites forest s into forest 0 (for
// every row that is no root in s, a union with its parent there: the trees of s become connected in 0); by density_kernels.h's invariant the root of a component is
// its smallest global row whatever the order.  density_roots_kernel flattens forest 0 into root[G];
// density_finish_sharded_kernel resolves a shard's local rows against it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "density_kernels.h"
#include "ids.h"
#include "join_between_kernels.h"
#include "tile128.h"

namespace mi {

// pass 1, stage 2: C candidates (ra, cb) (C <= the buffer's capacity) -> deg_a[ra] += 1, deg_col[cb] += 1 for the pairs
// within.  rows_b / deg_col count from the chunk's first row, which is B's local row col_off.
template <int NCH>
__global__ __launch_bounds__(256) void density_count_between_kernel(const float* __restrict__ rows_a, const float* __restrict__ rows_b,
                                                                    IdMap map_a, IdMap map_b, uint32_t col_off,
                                                                    const uint2* __restrict__ cand, uint32_t C, float max_dist,
                                                                    uint32_t* __restrict__ deg_a, uint32_t* __restrict__ deg_col,
                                                                    unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum and the ballot are cross-lane operations)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const float* ra = rows_a + (uint64_t)pr.x * DIM;
        const float* rb = rows_b + (uint64_t)pr.y * DIM;
        const bool b_asks = id_of_local(map_b, (uint64_t)col_off + pr.y) < id_of_local(map_a, pr.x);
        const float dist = pair_dist<NCH>(b_asks ? rb : ra, b_asks ? ra : rb, i);
        const bool keep = live && i == 0 && dist <= max_dist;
        const unsigned long long m = __ballot(keep);
        if (m == 0ull) continue;
        if (keep) {
            atomicAdd(deg_a + pr.x, 1u);
            atomicAdd(deg_col + pr.y, 1u);
        }
        if (lane == 0) atomicAdd(words + DW_WITHIN, (unsigned long long)__popcll(m));
    }
}

// pass 2, stage 1: cross_tiles_kernel (no bounds: everything qualifies) behind the activity test — tile (bi, bj) is left at
// once unless both blocks have bit 0 and one has bit 1.  act_a: A's blocks; act_b: the blocks of the column chunk.
template <int NCH>
__global__ __launch_bounds__(256) void density_cross_tiles_kernel(const uint16_t* __restrict__ mirror_a, const float* __restrict__ xx_a,
                                                                   const uint64_t* __restrict__ tomb_a, const uint8_t* __restrict__ act_a,
                                                                   uint32_t n_a, const uint16_t* __restrict__ mirror_b,
                                                                   const float* __restrict__ xx_b, const uint64_t* __restrict__ tomb_b,
                                                                   const uint8_t* __restrict__ act_b, uint32_t n_b, uint32_t br0,
                                                                   uint32_t bc0, float c, uint32_t cap, uint2* __restrict__ cand,
                                                                   unsigned long long* __restrict__ count) {
    pair_tile<NCH, false, true>(mirror_a, xx_a, tomb_a, act_a, n_a, mirror_b, xx_b, tomb_b, act_b, n_b, 0u, 0u, br0, bc0, c, cap, cand,
                                count);
}

// pass 2, stage 2: C candidates (ra, cb) -> unions of the core-core pairs within in `parent`, the row side's forest over
// GLOBAL rows, and bkey minima of the core-border pairs within, the core named by its global row.  deg_col / bkey_col count
// from the chunk's first row (B's local row col_off): B's own arrays, or a copy of its degrees and a chunk-local key array
// the host merges back.  A shard's self piece passes its own arrays on both sides.  (The candidates hold live rows only, so
// "core" is the degree test alone here.)
template <int NCH>
__global__ __launch_bounds__(256) void density_link_between_kernel(const float* __restrict__ rows_a, const float* __restrict__ rows_b,
                                                                   IdMap map_a, IdMap map_b, uint32_t col_off,
                                                                   const uint2* __restrict__ cand, uint32_t C, float max_dist,
                                                                   uint32_t min_pts, const uint32_t* __restrict__ deg_a,
                                                                   const uint32_t* __restrict__ deg_col, uint32_t* parent,
                                                                   unsigned long long* bkey_a, unsigned long long* bkey_col,
                                                                   unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum works across the 16 lanes of a group, which take every branch together)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const bool core_a = deg_a[pr.x] >= min_pts - 1u, core_b = deg_col[pr.y] >= min_pts - 1u;
        if (!live || !(core_a || core_b)) continue;
        const float* ra = rows_a + (uint64_t)pr.x * DIM;
        const float* rb = rows_b + (uint64_t)pr.y * DIM;
        const bool b_asks = id_of_local(map_b, (uint64_t)col_off + pr.y) < id_of_local(map_a, pr.x);
        const float dist = pair_dist<NCH>(b_asks ? rb : ra, b_asks ? ra : rb, i);
        if (i != 0 || !(dist <= max_dist)) continue;
        // (the global rows once more, for the few pairs that come this far: nothing of them is kept live across the rows' stream)
        const uint32_t ga = (uint32_t)id_of_local(map_a, pr.x), gb = (uint32_t)id_of_local(map_b, (uint64_t)col_off + pr.y);
        if (core_a && core_b) ds_union(parent, ga, gb, words);
        else if (core_a) atomicMin(bkey_col + pr.y, (unsigned long long)make_key(dist, ga));
        else atomicMin(bkey_a + pr.x, (unsigned long long)make_key(dist, gb));
    }
}

}  // namespace mi
