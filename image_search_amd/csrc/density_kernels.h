// density_kernels.h — device code of mi_knn_density and mi_knn_dbscan (density.hip): per-row neighbour counts within a cosine
// distance, and DBSCAN over them, on the join's tiles.  The pairs never leave the device.
//
// Let W be the pairs (a < b, d) mi_knn_near_pairs(max_dist, first_new = 0) reports.  Both passes below walk W strip by strip in
// the join's two stages (join_kernels.h: a bf16 tile stage that may only err on the side of MORE pairs, under the bound eps2,
// and the search's fp32 arithmetic deciding), so "within" is the join's decision bit for bit.
//
// Pass 1 (degrees).  Stage 1 is join_tiles_kernel itself.  Stage 2, density_count_kernel, is join_rescore_kernel (its distance
// as the function pair_dist of pair_kernels.h) with the compaction replaced by two integer adds: deg[a] += 1, deg[b] += 1.  Integer adds commute: the result is the same in any order.
//
// density_blocks_kernel.  Row r is a core iff it is live and deg[r] + 1 >= min_pts.  Per 128-row block one byte: bit 0 = some
// row has deg > 0, bit 1 = some row is a core.  parent[r] = r, bkey[r] = ~0.
//
// Pass 2 (links).  Stage 1, density_tiles_kernel, is the join's tile (pair_tile) with its SKIP test in front of the first
// load: the tile (bi, bj) is left at once unless both blocks have bit 0 and one has bit 1.  That skip is exact: a pair of W has both degrees
// > 0, and pass 2 uses only pairs with a core end.  Stage 2, density_link_kernel, reads the two core flags first; a pair with
// no core end is dropped without streaming its rows.  Otherwise the join's rescore decides, and a pair within
//   - with two core ends is a union in a lock-free disjoint-set forest over `parent` (below),
//   - with one core end is atomicMin(bkey[border], make_key(dist, core row)): the search's key order on the distance (-0 before
//     +0), then the smaller core row — a minimum, so the same in any arrival order.
//
// The forest (the union of ECL-CC: Jaiganesh & Burtscher, HPDC 2018).  Invariant: parent[x] <= x, equality exactly at a root.
// find() follows parents and, on its way, stores each node's grandparent into it (pointer jumping); union finds both roots and
// hangs the LARGER under the smaller with atomicCAS(parent + larger, larger, smaller), retrying from the value the CAS returned
// when it lost.  Every read of `parent` is a relaxed agent-scope atomic load, every write that CAS or a relaxed agent-scope
// atomic store; there are no plain accesses and no fences: nothing is published through `parent` but the values themselves.
// A stale read only names an older ancestor of the same tree (a node never leaves its tree and values only ever name
// ancestors), the CAS succeeds only on a current root, and since the smaller row is always the root, the final root of a
// component is its smallest row whatever the arrival order.  No workgroup waits for another.  Both loops carry a step cap
// (DENSITY_STEP_CAP, far above any path a forest of < 2^32 rows under pointer jumping shows); on expiry the error word is set
// and the host fails the call without writing anything.
//
// Pass 3, density_finish_kernel, runs behind the last strip — the kernel boundary is the only ordering needed — and resolves
// per row: root, cluster id, via, via_dist, through the IdMap (counts are deg itself); the summary is summed with one atomic per wave.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "join_kernels.h"
#include "tile128.h"

namespace mi {

constexpr uint32_t DENSITY_STEP_CAP = 1u << 24;
// the words of a call (unsigned long long each)
constexpr int DW_CAND = 0;      // candidates of the stage-1 launch in flight
constexpr int DW_WITHIN = 1;    // pairs within, pass 1
constexpr int DW_MERGED = 2;    // unions that merged
constexpr int DW_ERROR = 3;     // != 0: a step cap expired
constexpr int DW_SUMMARY = 4;   // clusters, core rows, border rows, noise rows
constexpr int DW_WORDS = 8;

__device__ __forceinline__ uint32_t ds_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ds_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as this thread sees it, halving the path on the way
__device__ __forceinline__ uint32_t ds_find(uint32_t* parent, uint32_t x, unsigned long long* words) {
    uint32_t cur = ds_load(parent + x);
    if (cur == x) return x;
    uint32_t prev = x;
    for (uint32_t step = 0;; ++step) {
        const uint32_t next = ds_load(parent + cur);
        if (next == cur) return cur;
        ds_store(parent + prev, next);   // the grandparent: an ancestor still
        prev = cur;
        cur = next;
        if (step >= DENSITY_STEP_CAP) { atomicAdd(words + DW_ERROR, 1ull); return cur; }
    }
}

// the trees of x and y become one; the smaller root stays a root
__device__ __forceinline__ void ds_union(uint32_t* parent, uint32_t x, uint32_t y, unsigned long long* words) {
    uint32_t a = ds_find(parent, x, words), b = ds_find(parent, y, words);
    for (uint32_t step = 0; a != b; ++step) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }   // a: the larger
        uint32_t seen = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            atomicAdd(words + DW_MERGED, 1ull);
            return;
        }
        // a was no root any more: go on from what it hangs under now (b may have lost its rank meanwhile too)
        a = ds_find(parent, seen, words);
        b = ds_find(parent, b, words);
        if (step >= DENSITY_STEP_CAP) { atomicAdd(words + DW_ERROR, 1ull); return; }
    }
}

// pass 1, stage 2: C candidate pairs (C <= the buffer's capacity) -> deg[a] += 1, deg[b] += 1 for the pairs within
template <int NCH>
__global__ __launch_bounds__(256) void density_count_kernel(const float* __restrict__ table, const uint2* __restrict__ cand, uint32_t C,
                                                            float max_dist, uint32_t* __restrict__ deg,
                                                            unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum and the ballot are cross-lane operations)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const float dist = pair_dist<NCH>(table + (uint64_t)pr.x * DIM, table + (uint64_t)pr.y * DIM, i);
        const bool keep = live && i == 0 && dist <= max_dist;
        const unsigned long long m = __ballot(keep);
        if (m == 0ull) continue;
        if (keep) {
            atomicAdd(deg + pr.x, 1u);
            atomicAdd(deg + pr.y, 1u);
        }
        if (lane == 0) atomicAdd(words + DW_WITHIN, (unsigned long long)__popcll(m));
    }
}

// one workgroup per 128-row block: act[block] = (some deg > 0) | (some core) << 1; parent[r] = r; bkey[r] = ~0
static __global__ __launch_bounds__(TILE) void density_blocks_kernel(const uint32_t* __restrict__ deg, const uint64_t* __restrict__ tomb,
                                                              uint32_t n_rows, uint32_t min_pts, uint32_t* __restrict__ parent,
                                                              unsigned long long* __restrict__ bkey, uint8_t* __restrict__ act) {
    __shared__ uint32_t bits;
    if (threadIdx.x == 0) bits = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * TILE + threadIdx.x;
    uint32_t mine = 0u;
    if (r < n_rows) {
        const uint32_t d = deg[r];
        parent[r] = r;
        bkey[r] = KEY_MAX;
        if (d > 0u) mine |= 1u;
        if (d >= min_pts - 1u && !tile_dead(tomb, r)) mine |= 2u;
    }
    const uint32_t any = (__ballot(mine & 1u) ? 1u : 0u) | (__ballot(mine & 2u) ? 2u : 0u);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(&bits, any);
    __syncthreads();
    if (threadIdx.x == 0) act[blockIdx.x] = (uint8_t)bits;
}

// pass 2, stage 1: join_tiles_kernel (first_new = 0) behind the activity test
template <int NCH>
__global__ __launch_bounds__(256) void density_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                             const uint64_t* __restrict__ tomb, const uint8_t* __restrict__ act,
                                                             uint32_t n_rows, uint32_t br0, uint32_t bc0, float c, uint32_t cap,
                                                             uint2* __restrict__ cand, unsigned long long* __restrict__ count) {
    pair_tile<NCH, true, true>(mirror, xx, tomb, act, n_rows, mirror, xx, tomb, act, n_rows, 0u, 0u, br0, bc0, c, cap, cand, count);
}

// pass 2, stage 2: C candidate pairs -> unions of core-core pairs within, bkey minima of core-border pairs within.  (The
// candidates hold live rows only, so "core" is the degree test alone here.)
template <int NCH>
__global__ __launch_bounds__(256) void density_link_kernel(const float* __restrict__ table, const uint2* __restrict__ cand, uint32_t C,
                                                           float max_dist, uint32_t min_pts, const uint32_t* __restrict__ deg,
                                                           uint32_t* parent, unsigned long long* __restrict__ bkey,
                                                           unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum works across the 16 lanes of a group, which take every branch together)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const bool core_a = deg[pr.x] >= min_pts - 1u, core_b = deg[pr.y] >= min_pts - 1u;
        if (!live || !(core_a || core_b)) continue;
        const float dist = pair_dist<NCH>(table + (uint64_t)pr.x * DIM, table + (uint64_t)pr.y * DIM, i);
        if (i != 0 || !(dist <= max_dist)) continue;
        if (core_a && core_b) ds_union(parent, pr.x, pr.y, words);
        else if (core_a) atomicMin(bkey + pr.y, (unsigned long long)make_key(dist, pr.x));
        else atomicMin(bkey + pr.x, (unsigned long long)make_key(dist, pr.y));
    }
}

// pass 3: per row, what the contract names (mi355clip.h).  via / via_dist may be null; counts are deg as it stands.
static __global__ __launch_bounds__(256) void density_finish_kernel(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ parent,
                                                             const unsigned long long* __restrict__ bkey,
                                                             const uint64_t* __restrict__ tomb, uint32_t n_rows, uint32_t min_pts,
                                                             IdMap map, uint64_t* __restrict__ cluster, uint64_t* __restrict__ via,
                                                             float* __restrict__ via_dist, unsigned long long* __restrict__ words) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int kind = -1;   // 0 a cluster's root, 1 another core, 2 border, 3 noise
    if (r < n_rows) {
        uint64_t cl = MI_KNN_NO_ID, v = MI_KNN_NO_ID;
        float vd = __uint_as_float(0x7F800000u);
        uint32_t cnt = 0u, from = 0xFFFFFFFFu;
        if (!tile_dead(tomb, r)) {
            cnt = deg[r];
            const unsigned long long key = bkey[r];
            if (cnt >= min_pts - 1u) { from = r; v = id_of_local(map, r); vd = 0.0f; kind = 1; }
            else if (key != KEY_MAX) { from = (uint32_t)key; v = id_of_local(map, from); vd = u32_to_dist((uint32_t)(key >> 32)); kind = 2; }
            else kind = 3;
        }
        if (from != 0xFFFFFFFFu) {
            // (parent is final: the walk reads, nothing writes any more; parent[x] < x off a root, so it ends within x steps)
            uint32_t x = from;
            for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
            cl = id_of_local(map, x);
            if (kind == 1 && x == r) kind = 0;
        }
        cluster[r] = cl;
        if (via) via[r] = v;
        if (via_dist) via_dist[r] = vd;
    }
    // clusters, core rows, border rows, noise rows: lane j < 4 adds word j, one atomic instruction per wave
    const unsigned long long m0 = __ballot(kind == 0), m1 = __ballot(kind == 0 || kind == 1), m2 = __ballot(kind == 2),
                             m3 = __ballot(kind == 3);
    if (lane < 4) {
        const unsigned long long m = lane == 0 ? m0 : lane == 1 ? m1 : lane == 2 ? m2 : m3;
        if (m != 0ull) atomicAdd(words + DW_SUMMARY + lane, (unsigned long long)__popcll(m));
    }
}

}  // namespace mi
