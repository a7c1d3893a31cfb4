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
// cross_rescore_kernel's arithmetic under its rule "the row with the smaller id is the query", the compaction replaced by
// deg_a[ra] += 1, deg_col[cb] += 1.
//
// Pass 2.  Stage 1, density_cross_tiles_kernel, is cross_tiles_kernel behind the activity test of density_tiles_kernel, the
// row block's byte and the column block's byte taken from two arrays.  Stage 2 of every piece, a shard's self piece
// included, is density_link_between_kernel: the forest it unites in spans the GLOBAL rows of the whole table (one forest per
// shard, on its device), a border key names the core by its global row.
//
// Behind the passes: density_forest_merge_kernel unites forest s into forest 0 (for every row that is no root in s, a union
// with its parent there: the trees of s become connected in 0); by density_kernels.h's invariant the root of a component is
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

// cross_rescore_kernel's arithmetic for one pair: q = the query's row, x = the row streamed against it; all 16 lanes of a
// group call it
template <int NCH>
__device__ __forceinline__ float between_pair_dist(const float* __restrict__ q, const float* __restrict__ x, int i) {
    const f32x4* pq = reinterpret_cast<const f32x4*>(q) + i;
    const f32x4* px = reinterpret_cast<const f32x4*>(x) + i;
    f32x4 qf[NCH];
#pragma unroll
    for (int t = 0; t < NCH; ++t) qf[t] = pq[16 * t];
    float sq;  // sqrt(q.q), same summation order as a row
    {
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
        sq = sqrtf(a.sumsq());
    }
    RowAcc<NCH> a; a.zero();
#pragma unroll
    for (int t = 0; t < NCH; ++t) a.step(qf[t], __builtin_nontemporal_load(px + 16 * t));
    const float d = a.dot(), s = a.sumsq();
    return 1.0f - d / (sq * sqrtf(s));
}

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
        const float dist = between_pair_dist<NCH>(b_asks ? rb : ra, b_asks ? ra : rb, i);
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
    constexpr int DIM = NCH * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t bi = br0 + blockIdx.y, bj = bc0 + blockIdx.x;
    {
        const uint32_t fa = act_a[bi], fb = act_b[bj];
        if (!((fa & fb & 1u) && ((fa | fb) & 2u))) return;   // no pair of W with a core end lies in this tile
    }
    const int tid = threadIdx.x;
    const TileFrag f = tile_frag();
    const int wr = f.wr, wc = f.wc, l31 = f.l31, lh = f.lh;
    float* wgt = reinterpret_cast<float*>(smem + TILE_IMGS);   // [0, 128): the tile's rows of A, [128, 256): its rows of B
    const uint32_t row0 = bi * TILE, col0 = bj * TILE;
    const float inf = __uint_as_float(0x7F800000u);

    {
        const bool is_col = tid >= TILE;
        const uint32_t r = (is_col ? col0 : row0) + (uint32_t)(tid & (TILE - 1));
        wgt[tid] = tile_weight<false>(is_col ? xx_b : xx_a, r, r < (is_col ? n_b : n_a), is_col ? tomb_b : tomb_a, r, -inf,
                                      __uint_as_float(0x7FC00000u));
    }

    const uint16_t *ga[4], *gb[4];
    tile_src<DIM>(ga, mirror_a, row0, n_a);
    tile_src<DIM>(gb, mirror_b, col0, n_b);
    f32x16 acc[2][2];
    tile_accumulate<NCH>(smem, f, ga, gb, acc);

    // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
    unsigned long long hit = 0ull;   // bit (2 ti + tj) * 16 + e
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ra0 = wr * 64 + ti * 32 + 8 * q + 4 * lh;
            const f32x4 wa = *reinterpret_cast<const f32x4*>(wgt + ra0);
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) {
                const int cb = wc * 64 + tj * 32 + l31;
                const float wb = wgt[TILE + cb];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = wa[j] * wb;
                    const bool ok = p == p && (!(acc[ti][tj][4 * q + j] < c * p) || fabsf(p) == inf);
                    if (ok) hit |= 1ull << ((2 * ti + tj) * 16 + 4 * q + j);
                }
            }
        }
    }
    tile_append(hit, f, row0, col0, cap, cand, count);
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
        const float dist = between_pair_dist<NCH>(b_asks ? rb : ra, b_asks ? ra : rb, i);
        if (i != 0 || !(dist <= max_dist)) continue;
        // (the global rows once more, for the few pairs that come this far: nothing of them is kept live across the rows' stream)
        const uint32_t ga = (uint32_t)id_of_local(map_a, pr.x), gb = (uint32_t)id_of_local(map_b, (uint64_t)col_off + pr.y);
        if (core_a && core_b) ds_union(parent, ga, gb, words);
        else if (core_a) atomicMin(bkey_col + pr.y, (unsigned long long)make_key(dist, ga));
        else atomicMin(bkey_a + pr.x, (unsigned long long)make_key(dist, gb));
    }
}

// ---- the small kernels between the pieces --------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void density_forest_init_kernel(uint32_t* __restrict__ parent, uint32_t n) {
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n; g += gridDim.x * 256) parent[g] = g;
}
// a staged chunk's degrees / border keys into the column shard's own, on its device (the shard is idle meanwhile)
static __global__ __launch_bounds__(256) void density_add_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n) {
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) dst[r] += src[r];
}
static __global__ __launch_bounds__(256) void density_min_kernel(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ src,
                                                          uint32_t n) {
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) dst[r] = min(dst[r], src[r]);
}

// other[i] = the parent of global row g0 + i in another shard's forest, copied here: where that is no root, a union in `parent`
static __global__ __launch_bounds__(256) void density_forest_merge_kernel(uint32_t* parent, const uint32_t* __restrict__ other, uint32_t g0,
                                                                   uint32_t n, unsigned long long* __restrict__ words) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t g = g0 + i, p = other[i];
        if (p != g) ds_union(parent, g, p, words);
    }
}

// root[g] = the root of g (parent is final: the walk reads, nothing writes any more; parent[x] < x off a root)
static __global__ __launch_bounds__(256) void density_roots_kernel(const uint32_t* __restrict__ parent, uint32_t* __restrict__ root, uint32_t n) {
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n; g += gridDim.x * 256) {
        uint32_t x = g;
        for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
        root[g] = x;
    }
}

// per local row of one shard what the contract names; `from` is a global row, root [G] the flattened forest.  via /
// via_dist may be null.  The summary: a cluster is counted by the shard that holds its root.
static __global__ __launch_bounds__(256) void density_finish_sharded_kernel(const uint32_t* __restrict__ deg,
                                                                     const unsigned long long* __restrict__ bkey,
                                                                     const uint64_t* __restrict__ tomb, const uint32_t* __restrict__ root,
                                                                     uint32_t n_rows, uint32_t min_pts, IdMap map,
                                                                     uint64_t* __restrict__ cluster, uint64_t* __restrict__ via,
                                                                     float* __restrict__ via_dist, unsigned long long* __restrict__ words) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int kind = -1;   // 0 a cluster's root, 1 another core, 2 border, 3 noise
    if (r < n_rows) {
        uint64_t cl = MI_KNN_NO_ID, v = MI_KNN_NO_ID;
        float vd = __uint_as_float(0x7F800000u);
        if (!tile_dead(tomb, r)) {
            const uint32_t g = (uint32_t)id_of_local(map, r);
            const unsigned long long key = bkey[r];
            if (deg[r] >= min_pts - 1u) {
                const uint32_t x = root[g];
                cl = x; v = g; vd = 0.0f;
                kind = x == g ? 0 : 1;
            } else if (key != KEY_MAX) {
                const uint32_t from = (uint32_t)key;
                cl = root[from]; v = from; vd = u32_to_dist((uint32_t)(key >> 32));
                kind = 2;
            } else {
                kind = 3;
            }
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
