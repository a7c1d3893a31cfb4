// join_kernels.h — device code of the threshold self-join (mi_knn_near_pairs): every pair of live rows (a < b) whose cosine
// distance is <= max_dist, "which of my images are there twice?".
//
// Two stages, the contract of the two-stage search (knn_kernels.h "bf16 mirror as prefilter"): a cheap first stage that may
// only err on the side of MORE pairs, and the fp32 arithmetic of knn_scan_kernel deciding.
//
// Stage 1 (join_tiles_kernel: pair_tile of pair_kernels.h as the self-join calls it), the matrix pipe.  S = M M^T over the bf16 mirror M (knn_mirror_kernel: rows rounded to
// nearest even, stored fp32 squared norms, -1 = marked), in tiles of 128 x 128 rows, only tiles on or above the diagonal.
// A workgroup of four waves owns one tile, a wave a 64 x 64 quadrant as 2 x 2 accumulators of v_mfma_f32_32x32x16_bf16;
// K runs in steps of 64 elements through a double-buffered LDS image (2 x 2 x 16 KiB).  The epilogue compares every
// accumulator with the threshold and appends the pairs that pass to a candidate buffer (one atomic per wave that has any).
//
// The bound eps2.  Both operands are rounded now: x~_j = x_j (1 + d_j), y~_j = y_j (1 + e_j), |d_j|, |e_j| <= u = 2^-8, so
// x~_j y~_j - x_j y_j = x_j y_j (d_j + e_j + d_j e_j) and |x~.y~ - x.y| <= (2u + u^2) sum |x_j y_j| <= (2u + u^2) |x| |y|
// (Cauchy-Schwarz): 2^-7 + 2^-16 on the cosine.  The products of two bf16 values are exact in fp32; the MFMA's fp32
// accumulation (any order) and the exact side's summation add <= 2 gamma_n each, gamma_n = (n + 8) 2^-24, the norms
// (stored against recomputed) another 2 gamma_n, divisions / square roots / the subtraction a few ulp of O(1) — the terms
// of the search's eps (knn_kernels.h), so
//     eps2 = 2^-7 + 2^-16 + 4.1 (dim + 8) 2^-24 + 2e-6        (8.02e-3 at dim 768),
// independent of the data; tests/test_join_bound.py drives rows built to sit at the rounding's worst case against it.
// A pair is a candidate when  coarse = 1 - acc / (sqrt(xx_a) sqrt(xx_b)) <= max_dist + eps2.  The epilogue evaluates this
// without the division, as  !(acc < (1 - max_dist - eps2) * (sqrt(xx_a) * sqrt(xx_b)))  — two roundings of relative 2^-24
// on a quantity of magnitude <= |x||y|, i.e. 1.2e-7 on the cosine, inside the 2e-6 above.  Rows the bound does not cover
// (marked in the mirror: a non-finite or > 3e38 element, a squared norm outside [1e-30, 1e30]) are candidates against
// every live row; deleted rows, rows beyond the table and columns below first_new never are.
//
// Stage 2 (join_rescore_kernel): one 16-lane group per candidate pair.  Row a is the query — its sqrt(q.q) from RowAcc as
// in knn_scan_kernel / knn_rescore_kernel — row b is streamed, dist = 1 - dot / (sq * sqrt(xx)): the value mi_knn_search
// with q = row a reports for row b, bit for bit.  That is pair_dist (pair_kernels.h), which the density kernels call; the three
// kernels that compact or mark pairs (this one, cross_rescore_kernel, diverse_rescore_kernel) keep it written out.  Pairs with dist <= max_dist (never a NaN) are compacted as (a, b, dist).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "pair_kernels.h"
#include "tile128.h"

namespace mi {

constexpr uint32_t JOIN_CAP_DEFAULT = PREF_CAP;

// grid (column blocks, row blocks): workgroup (x, y) takes tile (bi = br0 + y, bj = bc0 + x) and leaves at once when
// bj < bi.  c = 1 - (max_dist + eps2).  count: all candidates found, also those beyond cap (the caller then redoes the
// strip in smaller pieces); cand: the first `cap` of them as (a, b) local rows.
template <int NCH>
__global__ __launch_bounds__(256) void join_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                          const uint64_t* __restrict__ tomb, uint32_t n_rows, uint32_t first_new,
                                                          uint32_t br0, uint32_t bc0, float c, uint32_t cap,
                                                          uint2* __restrict__ cand, unsigned long long* __restrict__ count) {
    pair_tile<NCH, true, false>(mirror, xx, tomb, nullptr, n_rows, mirror, xx, tomb, nullptr, n_rows, 0u, first_new, br0, bc0, c, cap, cand,
                                count);
}

// stage 2: C candidate pairs (C <= the buffer's capacity: checked by the host before this runs) -> the pairs with exact
// distance <= max_dist as (a, b) + distance, unordered, *n_out of them (never more than C)
template <int NCH>
__global__ __launch_bounds__(256) void join_rescore_kernel(const float* __restrict__ table, const uint2* __restrict__ cand, uint32_t C,
                                                           float max_dist, uint2* __restrict__ out_pairs, float* __restrict__ out_dist,
                                                           uint32_t* __restrict__ n_out) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum and the append are cross-lane operations)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)pr.x * DIM) + i;
        const f32x4* pb = reinterpret_cast<const f32x4*>(table + (uint64_t)pr.y * DIM) + i;
        // (pair_dist of pair_kernels.h, written out: as a call it compiles to another register allocation here at NCH >= 8)
        f32x4 qf[NCH];
#pragma unroll
        for (int t = 0; t < NCH; ++t) qf[t] = pa[16 * t];
        float sq;  // sqrt(q.q), same summation order as a row
        {
            RowAcc<NCH> a; a.zero();
#pragma unroll
            for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
            sq = sqrtf(a.sumsq());
        }
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], __builtin_nontemporal_load(pb + 16 * t));
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
            out_pairs[at] = pr;
            out_dist[at] = dist;
        }
    }
}

}  // namespace mi
