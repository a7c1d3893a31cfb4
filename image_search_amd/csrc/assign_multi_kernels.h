// assign_multi_kernels.h — device code of mi_knn_assign_multi: for every row of the table the m nearest of C vectors, and
// only those within max_dist ("beach", "sunset" and "dog" at once; no tag at all for a photo that matches nothing).
//
// mi_knn_assign (assign_kernels.h) with "the best" replaced by "the m best": the same two stages, the same tile, the same
// bound.  mi_knn_assign and mi_knn_kmeans do not pass through here.
//
// Stage 1 (assign_multi_tiles_kernel).  The tile is assign_tiles_kernel's: four waves own 128 table rows and walk the
// column tiles of 128 vectors, a wave a 64 x 64 quadrant as 2 x 2 accumulators of v_mfma_f32_32x32x16_bf16, K in steps of 64
// through the double-buffered, xor-swizzled LDS image.  What differs is the row's threshold.  Each row keeps m
// ordered-integer SLOTS in LDS; slot j takes ds_max_i32 only from the columns c with c % m == j (c the vector's index), and
//     t_row = the minimum over the m slots,  -inf until every slot has been filled.
// A pair (row, c) is emitted iff  coarse >= t_row - 2 eps2  and it passes the join's distance test
//     !(acc < (1 - max_dist - eps2) w_a w_b)
// (max_dist = +inf makes the right-hand side -inf: the test passes everything that is there, as if it were skipped).
//
// Why that is a superset.  eps2 is the join's, unchanged (join_kernels.h), |coarse(c) - exact(c)| <= eps2 for every pair the
// mirror does not mark.  The m slots hold the coarse values of m DISTINCT columns (different residues), each >= t_row.
// Their exact values are >= t_row - eps2, so the exact m-th best is >= t_row - eps2, so every member of the exact top m has
// coarse >= t_row - 2 eps2.  Nothing in this depends on the visiting order or on which columns a launch sees, which is what
// the host's overflow pieces (a subset of the column tiles with fresh slots) need.  For m = 1 the one slot is
// assign_tiles_kernel's running maximum.  The distance test is the join's, a superset of dist <= max_dist by the same
// eps2.  A first pass that fixes the exact band and a second that emits would hand over fewer candidates at twice the MFMA
// work: DESIGN.md 5.17 has the counts and why the running form was kept.
// Marked rows / vectors (norm stored as -1) are candidates against everything that is there and stay out of the slots;
// deleted rows, rows beyond the table and the padding columns of the last tile never emit.
//
// Stage 2 (assign_multi_rescore_kernel): assign_rescore_kernel's arithmetic per candidate (the table row is the QUERY, the
// vector the streamed row: the search's distance bits), NaN and dist > max_dist dropped, then the key
// (dist_to_u32(dist) << 32 | label) goes down a chain of m 64-bit atomicMin:
//     old = atomicMin(&slot[r][j], key);  key = max(old, key);  on to slot j + 1.
// Slot 0 ends as the minimum of everything offered; what is carried on is everything else, so by induction slot j ends as
// the (j + 1)-th smallest whatever the interleaving (a candidate is offered once: an overflowing launch is not rescored).
// assign_multi_finalize_kernel (assign_multi.hip, its one user: search_many.hip includes this header for the rescore kernel)
// unpacks a strip's slots, pads behind the last hit and pads the deleted rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "tile128.h"

namespace mi {

constexpr int AMU_MAX_M = SLOT_MAX_M;                           // labels per row
// the tile's images + row weights, column 1 / w, column w, row thresholds + the rows' slots
constexpr int AMU_LDS = TILE_IMGS + 4 * TILE * 4 + SLOT_STRIDE * SLOT_MAX_M * 4;

// grid.x = row tiles: workgroup x takes rows of tile br0 + x against the column tiles [bc0, bc1).  1 <= m <= AMU_MAX_M.
// thr = 2 eps2, cdist = 1 - max_dist - eps2 (-inf = no threshold).  count: all candidates found, also those beyond cap
// (the caller then redoes the piece in smaller ones); cand: the first `cap` of them as (row, label).
template <int NCH>
__global__ __launch_bounds__(256, 2) void assign_multi_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                                  const uint64_t* __restrict__ tomb, uint32_t n_rows,
                                                                  const uint16_t* __restrict__ vmirror, const float* __restrict__ vxx,
                                                                  uint32_t n_vec, uint32_t m, uint32_t br0, uint32_t bc0, uint32_t bc1,
                                                                  float thr, float cdist, uint32_t cap, uint2* __restrict__ cand,
                                                                  unsigned long long* __restrict__ count) {
    constexpr int DIM = NCH * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const TileFrag f = tile_frag();
    const int wr = f.wr, wc = f.wc, l31 = f.l31, lh = f.lh;
    // weights: rows  > 0 = sqrt of the stored norm, -1 = marked, 0 = not there;  columns  colw > 0 = 1 / sqrt(norm), -1, 0
    // and colsq = sqrt(norm) where colw > 0
    float* roww = reinterpret_cast<float*>(smem + TILE_IMGS);
    float* colw = roww + TILE;
    float* colsq = colw + TILE;
    float* rowthr = colsq + TILE;
    int* slots = reinterpret_cast<int*>(rowthr + TILE);   // [slot][SLOT_STRIDE]: slot j of row r at j * stride + r
    const uint32_t row0 = (br0 + blockIdx.x) * TILE;

    if (tid < TILE) {
        const uint32_t r = row0 + (uint32_t)tid;
        roww[tid] = tile_weight<false>(xx, r, r < n_rows, tomb, r, -1.0f, 0.0f);
    }
    for (int j = tid; j < SLOT_STRIDE * (int)m; j += 256) slots[j] = TILE_ORD_NINF;
    const uint16_t *ga[4], *gb[4];
    tile_src<DIM>(ga, mirror, row0, n_rows);

#pragma unroll 1
    for (uint32_t bj = bc0; bj < bc1; ++bj) {
        const uint32_t col0 = bj * TILE;
        // (the previous tile's readers of the column weights and of the images passed the barrier that ends this iteration)
        if (tid < TILE) {
            const uint32_t cidx = col0 + (uint32_t)tid;
            colw[tid] = tile_weight<true>(vxx, cidx, cidx < n_vec, nullptr, 0u, -1.0f, 0.0f);
            colsq[tid] = tile_weight<false>(vxx, cidx, cidx < n_vec, nullptr, 0u, 0.0f, 0.0f);
        }
        tile_src<DIM>(gb, vmirror, col0, n_vec);
        f32x16 acc[2][2];
        tile_accumulate<NCH>(smem, f, ga, gb, acc);

        // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
        const int cl0 = wc * 64 + l31, cl1 = cl0 + 32;
        const float cw0 = colw[cl0], cw1 = colw[cl1];
        // (a) the tile's columns into the slots of their residues
        tile_slots_max(slots, roww, f, acc, col0, m, cw0, cw1);
        __syncthreads();
        // t_row (times w_a): the minimum over the row's slots
        if (tid < TILE) {
            int lowest = slots[tid];
            for (uint32_t j = 1; j < m; ++j) lowest = min(lowest, slots[j * SLOT_STRIDE + tid]);
            rowthr[tid] = tile_unord(lowest);
        }
        __syncthreads();
        // (b) what the thresholds cannot exclude
        const float cs0 = colsq[cl0], cs1 = colsq[cl1];
        unsigned long long hit = 0ull;   // bit (2 ti + tj) * 16 + e
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ra0 = wr * 64 + ti * 32 + 8 * q + 4 * lh;
                const f32x4 wa = *reinterpret_cast<const f32x4*>(roww + ra0);
                const f32x4 tr = *reinterpret_cast<const f32x4*>(rowthr + ra0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float bound = tr[j] - thr * wa[j];
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) {
                        const float cw = tj ? cw1 : cw0, cs = tj ? cs1 : cs0;
                        const float a = acc[ti][tj][4 * q + j];
                        const bool there = wa[j] != 0.0f && cw != 0.0f;
                        const bool ok = there && (wa[j] < 0.0f || cw < 0.0f || (!(a * cw < bound) && !(a < cdist * (wa[j] * cs))));
                        if (ok) hit |= 1ull << ((2 * ti + tj) * 16 + 4 * q + j);
                    }
                }
            }
        }
        tile_append(hit, f, row0, col0, cap, cand, count);
        __syncthreads();   // the column weights and the images may be overwritten
    }
}

// stage 2: n candidates (row, label) -> the m smallest keys of every row in slot[(row - row_base) * m + 0 .. m), ascending
template <int NCH>
__global__ __launch_bounds__(256) void assign_multi_rescore_kernel(const float* __restrict__ table, const float* __restrict__ vec,
                                                                   const uint2* __restrict__ cand, uint32_t n, uint32_t m,
                                                                   float max_dist, uint32_t row_base,
                                                                   unsigned long long* __restrict__ slot) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t c0 = group; c0 < ((n + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < n;
        const uint2 pr = cand[live ? c0 : 0];
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)pr.x * DIM) + i;
        const f32x4* pb = reinterpret_cast<const f32x4*>(vec + (uint64_t)pr.y * DIM) + i;
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
        for (int t = 0; t < NCH; ++t) a.step(qf[t], pb[16 * t]);
        const float d = a.dot(), s = a.sumsq();
        const float dist = 1.0f - d / (sq * sqrtf(s));
        if (live && i == 0 && dist <= max_dist) {   // (a NaN compares false: never a label)
            unsigned long long key = (unsigned long long)make_key(dist, pr.y);
            unsigned long long* p = slot + (uint64_t)(pr.x - row_base) * m;
            for (uint32_t j = 0; j < m; ++j) {
                const unsigned long long old = atomicMin(p + j, key);
                if (old > key) key = old;
                if (key == KEY_MAX) break;   // the slot was empty: nothing to carry on
            }
        }
    }
}

}  // namespace mi
