// density_levels_kernels.h — device code of mi_knn_density_levels and mi_knn_dbscan_levels (density_levels.hip): what L calls
// of mi_knn_density / mi_knn_dbscan at ascending distances d[0] < ... < d[L - 1] return, from the two tile passes one call runs.
// The tiles and the pair distance are pair_kernels.h's (pair_tile, pair_dist), the forest is density_kernels.h's, unedited.
//
// Why one pass serves every level.  Let W_l be the pairs mi_knn_near_pairs(d[l]) reports.  Stage 1 (join_tiles_kernel under
// c = 1 - (d[L - 1] + eps2)) passes a superset of W_{L-1}, and W_l is a subset of W_{L-1} for every l, since dist <= d[l]
// implies dist <= d[L - 1].  Stage 2 computes pair_dist (pair_kernels.h), the single call's fp32 bits, which do not depend on the
// threshold; lv = the number of levels with !(dist <= d[l]) is, the thresholds ascending, the first level with dist <= d[lv]:
// the same float compare the single call makes, so the pair is in W_m exactly for m >= lv (a NaN: lv = L, in no level).
//
// Pass 1.  density_count_levels_kernel adds 1 to the exclusive bins degbin[lv][a] and degbin[lv][b]: one pair of integer
// atomics per pair, not one per level; the per-level "within" words are exclusive bins too (the host sums them).
//
// density_levels_blocks_kernel, per 128-row block: the row's bins are prefix-summed over the levels in place, so
// deg[l][r] = the pairs of W_l that contain r, mi_knn_density(d[l])'s count.  core_from[r] = the smallest level at which r is
// live and deg[l][r] + 1 >= min_pts (L if none): deg[.][r] does not fall with l, so r is a core at exactly the levels
// >= core_from[r].  parent[l][r] = r, bkey[l][r] = ~0 for every level.  The activity byte is the top level's: bit 0 = some
// deg[L - 1] > 0, bit 1 = some core at L - 1.  density_tiles_kernel's skip stays exact for EVERY level: a pair of W_l is a pair of
// W_{L-1}, so both its rows have deg[L - 1] > 0 (deg[l] <= deg[L - 1]), and a core end at level l is a core at L - 1; a tile
// that holds a pair some level uses therefore passes the top level's test.
//
// Pass 2.  Stage 1 is density_tiles_kernel with c of the top level.  Stage 2, density_link_levels_kernel, loads the two
// core_from bytes first and drops a pair with no core end at any level without streaming its rows.  Otherwise dist once, lv,
// and for every level m >= max(lv, the smaller core_from): both ends core at m -> ds_union in forest m; one -> atomicMin(bkey[m]
// + border, make_key(dist, core row)).  Level m thus sees exactly the unions and minima density_link_kernel applies in a call at
// d[m]; both are order-free (density_kernels.h), so forest m and bkey[m] end as that call's.  ds_find / ds_union take this
// unit's words: DWL_MERGED and DWL_ERROR sit where DW_MERGED and DW_ERROR do, so one word sums the merges of all levels and one
// the expired step caps.
//
// density_levels_finish_kernel runs over (row, level) and is density_finish_kernel's resolution on slice l.
//
// Device memory of a call: L * (4 + 4 + 8) bytes per row (deg, parent, bkey) + 1 (core_from), one byte per block, and the result
// arrays; all from Scratch, freed with the call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "density_kernels.h"
#include "density_levels_host.h"

namespace mi {

// the words of a call (unsigned long long each); a layout of its own, not DW_* stretched
constexpr int DWL_CAND = 0;      // candidates of the stage-1 launch in flight
constexpr int DWL_MERGED = 2;    // unions that merged, all levels (ds_union's DW_MERGED)
constexpr int DWL_ERROR = 3;     // != 0: a step cap expired (ds_find's / ds_union's DW_ERROR)
constexpr int DWL_WITHIN = 8;    // [MI_KNN_LEVELS_MAX]: pairs whose first level is l
constexpr int DWL_SUMMARY = 16;  // [MI_KNN_LEVELS_MAX][4]: clusters, core rows, border rows, noise rows
constexpr int DWL_WORDS = DWL_SUMMARY + 4 * MI_KNN_LEVELS_MAX;
static_assert(DWL_MERGED == DW_MERGED && DWL_ERROR == DW_ERROR, "ds_find / ds_union write DW_MERGED and DW_ERROR of the words they are given");
static_assert(DWL_CAND == DW_CAND, "DensityStage1 (density_call.h) is handed the word; both layouts keep it first");
static_assert(DWL_CAND != DWL_MERGED && DWL_CAND != DWL_ERROR && DWL_WITHIN > DWL_ERROR, "the words must not overlap");

// density_level_of_host on the device: the levels that fail the single call's compare
__device__ __forceinline__ uint32_t density_level_of(const DensityLevels& lv, float dist) {
    uint32_t l = 0;
#pragma unroll
    for (int j = 0; j < MI_KNN_LEVELS_MAX; ++j) l += ((uint32_t)j < lv.n && !(dist <= lv.d[j])) ? 1u : 0u;
    return l;
}

// pass 1, stage 2: C candidate pairs (C <= the buffer's capacity) -> degbin[lv][a] += 1, degbin[lv][b] += 1 for the pairs
// within the top level.  degbin: [lv.n][n_rows]
template <int NCH>
__global__ __launch_bounds__(256) void density_count_levels_kernel(const float* __restrict__ table, const uint2* __restrict__ cand,
                                                                   uint32_t C, DensityLevels lv, uint32_t n_rows,
                                                                   uint32_t* __restrict__ degbin, unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum and the ballots are cross-lane operations)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const float dist = pair_dist<NCH>(table + (uint64_t)pr.x * DIM, table + (uint64_t)pr.y * DIM, i);
        const uint32_t l = density_level_of(lv, dist);
        const bool keep = live && i == 0 && l < lv.n;
        if (__ballot(keep) == 0ull) continue;
        if (keep) {
            uint32_t* bin = degbin + (uint64_t)l * n_rows;
            atomicAdd(bin + pr.x, 1u);
            atomicAdd(bin + pr.y, 1u);
        }
        // lane j < L adds the wave's pairs of level j: one atomic instruction per wave
        uint32_t mine = 0u;
        for (uint32_t j = 0; j < lv.n; ++j) {
            const uint32_t n = (uint32_t)__popcll(__ballot(keep && l == j));
            if ((uint32_t)lane == j) mine = n;
        }
        if (mine != 0u) atomicAdd(words + DWL_WITHIN + lane, (unsigned long long)mine);
    }
}

// one workgroup per 128-row block: the bins -> cumulative degrees in place, core_from, parent[l][r] = r, bkey[l][r] = ~0, and
// the block's activity byte from the top level.  parent == null: the degrees only (mi_knn_density_levels).
static __global__ __launch_bounds__(TILE) void density_levels_blocks_kernel(uint32_t* __restrict__ deg, const uint64_t* __restrict__ tomb,
                                                                            uint32_t n_rows, uint32_t n_levels, uint32_t min_pts,
                                                                            uint32_t* __restrict__ parent,
                                                                            unsigned long long* __restrict__ bkey,
                                                                            uint8_t* __restrict__ core_from, uint8_t* __restrict__ act) {
    __shared__ uint32_t bits;
    if (threadIdx.x == 0) bits = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * TILE + threadIdx.x;
    uint32_t mine = 0u;
    if (r < n_rows) {
        const bool alive = !tile_dead(tomb, r);
        uint32_t run = 0u, from = n_levels;
        for (uint32_t l = 0; l < n_levels; ++l) {
            const uint64_t at = (uint64_t)l * n_rows + r;
            run += deg[at];
            deg[at] = run;
            if (parent) {
                if (from == n_levels && alive && run >= min_pts - 1u) from = l;
                parent[at] = r;
                bkey[at] = KEY_MAX;
            }
        }
        if (parent) core_from[r] = (uint8_t)from;
        if (run > 0u) mine |= 1u;
        if (from < n_levels) mine |= 2u;
    }
    if (!parent) return;   // (uniform: a kernel argument)
    const uint32_t any = (__ballot(mine & 1u) ? 1u : 0u) | (__ballot(mine & 2u) ? 2u : 0u);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(&bits, any);
    __syncthreads();
    if (threadIdx.x == 0) act[blockIdx.x] = (uint8_t)bits;
}

// pass 2, stage 2: C candidate pairs -> per level m the pair lies within: a union in forest m when both ends are cores at m,
// a bkey[m] minimum when one is.  (The candidates hold live rows only; core_from already knows of the deleted ones.)
template <int NCH>
__global__ __launch_bounds__(256) void density_link_levels_kernel(const float* __restrict__ table, const uint2* __restrict__ cand, uint32_t C,
                                                                  DensityLevels lv, uint32_t n_rows, const uint8_t* __restrict__ core_from,
                                                                  uint32_t* parent, unsigned long long* __restrict__ bkey,
                                                                  unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum works across the 16 lanes of a group, which take every branch together)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const uint32_t fa = core_from[pr.x], fb = core_from[pr.y];
        const uint32_t lo = fa < fb ? fa : fb, hi = fa < fb ? fb : fa;   // one end is a core from lo on, both from hi on
        if (!live || lo >= lv.n) continue;
        const float dist = pair_dist<NCH>(table + (uint64_t)pr.x * DIM, table + (uint64_t)pr.y * DIM, i);
        const uint32_t l0 = density_level_of(lv, dist);
        if (i != 0 || l0 >= lv.n) continue;
        // below hi the end that turns core later is the border row
        const uint32_t core = fa < fb ? pr.x : pr.y, border = fa < fb ? pr.y : pr.x;
        const unsigned long long key = (unsigned long long)make_key(dist, core);
        for (uint32_t m = l0 > lo ? l0 : lo; m < lv.n; ++m) {
            const uint64_t at = (uint64_t)m * n_rows;
            if (m >= hi) ds_union(parent + at, pr.x, pr.y, words);
            else atomicMin(bkey + at + border, key);
        }
    }
}

// pass 3 over (row, level = blockIdx.y): density_finish_kernel's resolution into slice l.  via / via_dist may be null; counts
// are the cumulative deg as the blocks kernel left it.
static __global__ __launch_bounds__(256) void density_levels_finish_kernel(const uint32_t* __restrict__ parent,
                                                                           const unsigned long long* __restrict__ bkey,
                                                                           const uint8_t* __restrict__ core_from,
                                                                           const uint64_t* __restrict__ tomb, uint32_t n_rows, IdMap map,
                                                                           uint64_t* __restrict__ cluster, uint64_t* __restrict__ via,
                                                                           float* __restrict__ via_dist, unsigned long long* __restrict__ words) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const uint64_t base = (uint64_t)l * n_rows;
    int kind = -1;   // 0 a cluster's root, 1 another core, 2 border, 3 noise
    if (r < n_rows) {
        uint64_t cl = MI_KNN_NO_ID, v = MI_KNN_NO_ID;
        float vd = __uint_as_float(0x7F800000u);
        uint32_t from = 0xFFFFFFFFu;
        if (!tile_dead(tomb, r)) {
            const unsigned long long key = bkey[base + r];
            if (core_from[r] <= l) { from = r; v = id_of_local(map, r); vd = 0.0f; kind = 1; }
            else if (key != KEY_MAX) { from = (uint32_t)key; v = id_of_local(map, from); vd = u32_to_dist((uint32_t)(key >> 32)); kind = 2; }
            else kind = 3;
        }
        if (from != 0xFFFFFFFFu) {
            // (parent is final: the walk reads, nothing writes any more; parent[x] < x off a root, so it ends within x steps)
            const uint32_t* p_l = parent + base;
            uint32_t x = from;
            for (uint32_t p = p_l[x]; p != x; p = p_l[x]) x = p;
            cl = id_of_local(map, x);
            if (kind == 1 && x == r) kind = 0;
        }
        cluster[base + r] = cl;
        if (via) via[base + r] = v;
        if (via_dist) via_dist[base + r] = vd;
    }
    // clusters, core rows, border rows, noise rows of level l: lane j < 4 adds word j, one atomic instruction per wave
    const unsigned long long m0 = __ballot(kind == 0), m1 = __ballot(kind == 0 || kind == 1), m2 = __ballot(kind == 2),
                             m3 = __ballot(kind == 3);
    if (lane < 4) {
        const unsigned long long m = lane == 0 ? m0 : lane == 1 ? m1 : lane == 2 ? m2 : m3;
        if (m != 0ull) atomicAdd(words + DWL_SUMMARY + 4 * l + lane, (unsigned long long)__popcll(m));
    }
}

}  // namespace mi
