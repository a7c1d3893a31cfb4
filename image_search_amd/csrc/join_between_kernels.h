// join_between_kernels.h — device code of the threshold join of TWO row sets (mi_knn_near_pairs_between: "which pictures of
// that other library do I already have?"; mi_knn_sharded_near_pairs: the pairs whose rows live in different shards).  The
// kernels of join_kernels.h with a row operand (A, where the work runs) and a column operand (B) that come from different
// tables: pair_tile and pair_dist (pair_kernels.h) keep the two apart, the self-join passes one table as both.
//
// Stage 1 (cross_tiles_kernel).  S = M_a M_b^T over the two bf16 mirrors, every tile of the rectangle the host launches:
// there is no diagonal, every element of a tile may be a pair.  The bound eps2 (join_kernels.h) is a bound on two
// INDEPENDENTLY rounded operands — x~_j = x_j (1 + d_j), y~_j = y_j (1 + e_j) — and on two stored norms; nothing in its
// derivation uses that x and y are rows of one table, so it holds unchanged and the candidates are a superset of the pairs
// within max_dist.  The weights are the self-join's: -inf for a row the mirror marked (a candidate against everything live
// on the other side), NaN for a row that is deleted or beyond its table.  (fn_a, fn_b): element (ra, cb) can be a candidate
// only if ra >= fn_a or cb >= fn_b — the sharded join's "the larger id is >= first_new", both sides as local rows.  The host
// launches no tile that lies wholly below both bounds; the test here serves the tiles that straddle one.
//
// Stage 2 (cross_rescore_kernel): one 16-lane group per candidate (ra, cb).  Fixed mode: the row of A is the query.  Id-ordered
// mode: the row with the smaller id (id_of_local of either side's IdMap) is the query — what the single-table join does with
// the same two rows, where a < b are ids — so the distance has the bits mi_knn_search(q = the smaller-id row) reports for the
// other row.  Survivors (dist <= max_dist, never a NaN) are compacted as (ra, col_off + cb, dist): local rows, the host maps
// them to ids and puts the smaller id first.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "join_kernels.h"   // JOIN_LDS: the same LDS layout (the tile's images + the rows' weights)
#include "tile128.h"

namespace mi {

// grid (column blocks, row blocks): workgroup (x, y) takes tile (bi = br0 + y, bj = bc0 + x) of rows of A against rows of B.
// c = 1 - (max_dist + eps2).  count: all candidates found, also those beyond cap (the caller then redoes the rectangle in
// smaller pieces); cand: the first `cap` of them as (ra, cb) local rows.
template <int NCH>
__global__ __launch_bounds__(256) void cross_tiles_kernel(const uint16_t* __restrict__ mirror_a, const float* __restrict__ xx_a,
                                                           const uint64_t* __restrict__ tomb_a, uint32_t n_a,
                                                           const uint16_t* __restrict__ mirror_b, const float* __restrict__ xx_b,
                                                           const uint64_t* __restrict__ tomb_b, uint32_t n_b, uint32_t fn_a,
                                                           uint32_t fn_b, uint32_t br0, uint32_t bc0, float c, uint32_t cap,
                                                           uint2* __restrict__ cand, unsigned long long* __restrict__ count) {
    pair_tile<NCH, false, false>(mirror_a, xx_a, tomb_a, nullptr, n_a, mirror_b, xx_b, tomb_b, nullptr, n_b, fn_a, fn_b, br0, bc0, c, cap,
                                 cand, count);
}

// stage 2: C candidates (ra, cb) (C <= the buffer's capacity: checked by the host before this runs) -> the pairs with exact
// distance <= max_dist as (ra, col_off + cb) + distance, unordered, *n_out of them (never more than C).  rows_a: A's fp32
// rows; rows_b: the fp32 rows of B the candidates' columns count from (B's table, or a staged chunk of it that starts at
// B's local row col_off).  by_id: the row with the smaller id is the query (ids equal: A's), else always A's.
template <int NCH>
__global__ __launch_bounds__(256) void cross_rescore_kernel(const float* __restrict__ rows_a, const float* __restrict__ rows_b,
                                                            IdMap map_a, IdMap map_b, uint32_t col_off, int by_id,
                                                            const uint2* __restrict__ cand, uint32_t C, float max_dist,
                                                            uint2* __restrict__ out_pairs, float* __restrict__ out_dist,
                                                            uint32_t* __restrict__ n_out) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum and the append are cross-lane operations)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const float* ra = rows_a + (uint64_t)pr.x * DIM;
        const float* rb = rows_b + (uint64_t)pr.y * DIM;
        const bool b_asks = by_id && id_of_local(map_b, (uint64_t)col_off + pr.y) < id_of_local(map_a, pr.x);
        const f32x4* pq = reinterpret_cast<const f32x4*>(b_asks ? rb : ra) + i;   // the query
        const f32x4* px = reinterpret_cast<const f32x4*>(b_asks ? ra : rb) + i;   // the row streamed against it
        // (pair_dist of pair_kernels.h, written out: as a call it compiles to another register allocation here at NCH >= 8)
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
        const float dist = 1.0f - d / (sq * sqrtf(s));
        const bool keep = live && i == 0 && dist <= max_dist;
        const unsigned long long m = __ballot(keep);
        if (m == 0ull) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(n_out, (uint32_t)__popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (keep) {
            const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            out_pairs[at] = make_uint2(pr.x, col_off + pr.y);
            out_dist[at] = dist;
        }
    }
}

}  // namespace mi
