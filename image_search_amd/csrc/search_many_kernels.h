// search_many_kernels.h — device code of mi_knn_search_many / mi_knn_neighbors: for each of many query vectors the k <= 16
// nearest live rows of the table, exact, with the search's bits.  The kNN graph is the case "the queries are the table's own
// rows", the per-label top k the case "the queries are the label vectors".
//
// mi_knn_assign_multi turned round: there every table row looked for its m nearest of C <= 65 536 host vectors and one
// workgroup per row tile walked all column tiles; here the COLUMNS are the table (millions of rows, deleted ones among
// them) and the rows are a few hundred to a few ten thousand queries, so the column tiles are spread over the machine:
//
// Stage 1 (search_many_tiles_kernel), grid = row tile x column SEGMENT, two passes over the tile product.  The tile is
// assign_multi_tiles_kernel's: four waves, 128 x 128, a wave a 64 x 64 quadrant as 2 x 2 accumulators of
// v_mfma_f32_32x32x16_bf16, K in steps of 64 through the double-buffered, xor-swizzled LDS image.
//   threshold pass (EMIT = false): each workgroup keeps the m residue slots per row in LDS for the tiles it visits (slot j =
//     the running maximum of the coarse value over the columns c with c % m == j, c the table's row index) and folds them
//     into the strip's global slots [strip rows][m] with ordered-int atomicMax when its segment ends.  Nothing is emitted.
//     It may visit every `step`-th column tile only: see below.
//   emit pass (EMIT = true): t_row = the minimum over the row's m global slots (-inf while one is empty); the pair
//     (row, c) is emitted iff  coarse >= t_row - 2 eps2,  by the join's ballot / prefix / one-atomic-per-wave append.  No
//     slots in LDS: 66 KB per workgroup instead of 74.
//
// Why that is a superset of every row's exact top m (5.17's argument, unchanged).  eps2 is the join's, |coarse - exact| <=
// eps2 for every pair the mirror does not mark.  The m global slots hold coarse values of m DISTINCT live unmarked columns
// (different residues), each >= t_row, so m columns have exact >= t_row - eps2, so the exact m-th best is >= t_row - eps2,
// so every member of the exact top m has coarse >= t_row - 2 eps2.  The argument does not ask WHICH columns filled the
// slots: a threshold pass over a sample of the column tiles gives a lower, still valid t_row (more candidates, less MFMA
// work), and a strip's thresholds stay valid for every piece the host cuts the emit pass into.
// Marked rows / columns (norm stored as -1) are candidates against everything that is there and stay out of the slots;
// deleted columns, deleted query rows (mi_knn_neighbors), rows beyond the strip and the padding of the last tile have
// weight 0: they never emit and never enter a slot.
//
// Stage 2 is assign_multi_rescore_kernel as it stands (table = the fp32 queries, vec = the table: the query is the query,
// the table row is streamed — the search's distance bits; NaN dropped; the m smallest keys per query through the chain of
// 64-bit atomicMin).  search_many_finalize_kernel unpacks a strip's slots into ids / distances, drops a row's own entry
// for mi_knn_neighbors and pads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "assign_multi_kernels.h"   // stage 2: assign_multi_rescore_kernel

namespace mi {

constexpr int SMY_LDS_EMIT = TILE_IMGS + 4 * TILE * 4;                                   // images + weights + thresholds
constexpr int SMY_LDS_THR = SMY_LDS_EMIT + SLOT_STRIDE * SLOT_MAX_M * 4;                 // + the rows' slots

// grid = (row tiles, segments).  Workgroup (x, y): query rows of tile br0 + x (strip-local rows, n_q of them; row r is the
// table's row q_local0 + r where q_tomb is given) against the column tiles bc0 + i * step, i in [y n_i / segments,
// (y + 1) n_i / segments); segments <= n_i.  1 <= m <= AMU_MAX_M.  thr = 2 eps2.  gslot: [strip rows][m] ordered ints.
// EMIT: count = all candidates found, also those beyond cap; cand = the first `cap` of them as (strip-local row, column).
template <int NCH, bool EMIT>
__global__ __launch_bounds__(256, 2) void search_many_tiles_kernel(const uint16_t* __restrict__ qmirror, const float* __restrict__ qxx,
                                                                 const uint64_t* __restrict__ q_tomb, uint32_t q_local0, uint32_t n_q,
                                                                 const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                                 const uint64_t* __restrict__ tomb, uint32_t n_cols, uint32_t m,
                                                                 uint32_t br0, uint32_t bc0, uint32_t step, uint32_t n_i, float thr, int* __restrict__ gslot, uint32_t cap,
                                                                 uint2* __restrict__ cand, unsigned long long* __restrict__ count) {
    constexpr int DIM = NCH * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const TileFrag f = tile_frag();
    const int wr = f.wr, wc = f.wc, l31 = f.l31, lh = f.lh;
    // weights: rows  > 0 = sqrt of the stored norm, -1 = marked, 0 = not there;  columns  colw > 0 = 1 / sqrt(norm), -1, 0
    float* roww = reinterpret_cast<float*>(smem + TILE_IMGS);
    float* colw = roww + TILE;
    float* rowthr = colw + TILE;                              // (EMIT) t_row times w_a
    int* slots = reinterpret_cast<int*>(rowthr + 2 * TILE);   // (!EMIT) [slot][SLOT_STRIDE]
    const uint32_t row0 = (br0 + blockIdx.x) * TILE;
    const uint32_t i0 = (uint32_t)((uint64_t)blockIdx.y * n_i / gridDim.y), i1 = (uint32_t)((uint64_t)(blockIdx.y + 1) * n_i / gridDim.y);

    if (tid < TILE) {
        const uint32_t r = row0 + (uint32_t)tid;
        roww[tid] = tile_weight<false>(qxx, r, r < n_q, q_tomb, q_local0 + r, -1.0f, 0.0f);
        if (EMIT) {
            int lowest = TILE_ORD_NINF;
            if (r < n_q) {
                lowest = gslot[(size_t)r * m];
                for (uint32_t j = 1; j < m; ++j) lowest = min(lowest, gslot[(size_t)r * m + j]);
            }
            rowthr[tid] = tile_unord(lowest);
        }
    }
    if (!EMIT)
        for (int j = tid; j < SLOT_STRIDE * (int)m; j += 256) slots[j] = TILE_ORD_NINF;
    const uint16_t *ga[4], *gb[4];
    tile_src<DIM>(ga, qmirror, row0, n_q);

#pragma unroll 1
    for (uint32_t it = i0; it < i1; ++it) {
        const uint32_t col0 = (bc0 + it * step) * TILE;
        // (the previous tile's readers of the column weights and of the images passed the barrier that ends this iteration)
        if (tid < TILE) {
            const uint32_t cidx = col0 + (uint32_t)tid;
            colw[tid] = tile_weight<true>(xx, cidx, cidx < n_cols, tomb, cidx, -1.0f, 0.0f);
        }
        tile_src<DIM>(gb, mirror, col0, n_cols);
        f32x16 acc[2][2];
        tile_accumulate<NCH>(smem, f, ga, gb, acc);

        // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
        const int cl0 = wc * 64 + l31, cl1 = cl0 + 32;
        const float cw0 = colw[cl0], cw1 = colw[cl1];
        if (!EMIT) {
            // the tile's columns into the slots of their residues
            tile_slots_max(slots, roww, f, acc, col0, m, cw0, cw1);
        } else {
            // what the thresholds cannot exclude
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
                            const float cw = tj ? cw1 : cw0;
                            const float a = acc[ti][tj][4 * q + j];
                            const bool there = wa[j] != 0.0f && cw != 0.0f;
                            const bool ok = there && (wa[j] < 0.0f || cw < 0.0f || !(a * cw < bound));
                            if (ok) hit |= 1ull << ((2 * ti + tj) * 16 + 4 * q + j);
                        }
                    }
                }
            }
            tile_append(hit, f, row0, col0, cap, cand, count);
        }
        __syncthreads();   // the column weights and the images may be overwritten
    }
    if (!EMIT) {
        // the segment's slots into the strip's (vector atomics on global memory; an empty slot changes nothing)
        for (int j = tid; j < TILE * (int)m; j += 256) {
            const int row = j & (TILE - 1), sl = j / TILE;
            const int v = slots[sl * SLOT_STRIDE + row];
            const uint32_t r = row0 + (uint32_t)row;
            if (r < n_q && v > TILE_ORD_NINF) atomicMax(gslot + (size_t)r * m + sl, v);
        }
    }
}

// a strip's slots ([n_local][m] keys, ascending, KEY_MAX = none; key = distance key << 32 | local table row) -> ids / dist
// [n_local][k].  self_drop = 0: k = m.  self_drop = 1 (mi_knn_neighbors): k = m - 1, query r is the table's local row
// q_local0 + r: its own entry is removed, or, where that is absent, the last one; a deleted query row gets padding.
// *hits += the entries written that are not padding.
__global__ __launch_bounds__(256) void search_many_finalize_kernel(const unsigned long long* __restrict__ slot,
                                                                   const uint64_t* __restrict__ q_tomb, uint32_t q_local0,
                                                                   uint32_t n_local, uint32_t m, uint32_t self_drop, IdMap map,
                                                                   uint64_t* __restrict__ idx, float* __restrict__ dist,
                                                                   unsigned long long* __restrict__ hits) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    uint32_t written = 0;
    if (r < n_local) {
        const uint32_t k = m - self_drop, self = q_local0 + r;
        const bool dead = q_tomb && ((q_tomb[self >> 6] >> (self & 63)) & 1ull);
        const unsigned long long* p = slot + (size_t)r * m;
        uint64_t* oi = idx + (size_t)r * k;
        float* od = dist + (size_t)r * k;
        for (uint32_t j = 0; j < m && written < k && !dead; ++j) {
            const unsigned long long key = p[j];
            if (key == KEY_MAX) break;
            if (self_drop && (uint32_t)key == self) continue;
            oi[written] = id_of_local(map, (uint32_t)key);
            od[written] = u32_to_dist((uint32_t)(key >> 32));
            ++written;
        }
        for (uint32_t j = written; j < k; ++j) {
            oi[j] = MI_KNN_NO_ID;
            od[j] = __uint_as_float(0x7F800000u);
        }
    }
    // one atomic per wave
    uint32_t sum = written;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum != 0u) atomicAdd(hits, (unsigned long long)sum);
}

}  // namespace mi
