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

// the shared device code (the tile constants, the rescore, knn_mirror_kernel, the keys, IdMap) through a namespace of its
// own: see join_kernels.h
namespace mi_search_many {
#include "assign_multi_kernels.h"
}

namespace mi_search_many {
namespace mi_assign_multi {
namespace mi {

constexpr int SMY_LDS_EMIT = 4 * AMU_IMG + 4 * AMU_TILE * 4;                             // images + weights + thresholds
constexpr int SMY_LDS_THR = SMY_LDS_EMIT + AMU_SLOT_STRIDE * AMU_MAX_M * 4;              // + the rows' slots
constexpr int SMY_ORD_NINF = (int)0x807FFFFFu;                                           // amu_ord(-inf): an empty slot

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
    static_assert(NCH % 2 == 0, "rows of whole 256-byte bf16 chunks (the mirror's own condition)");
    constexpr int DIM = NCH * 64, NK = DIM / AMU_KC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const int wr = wib >> 1, wc = wib & 1, l31 = lane & 31, lh = lane >> 5;
    // weights: rows  > 0 = sqrt of the stored norm, -1 = marked, 0 = not there;  columns  colw > 0 = 1 / sqrt(norm), -1, 0
    float* roww = reinterpret_cast<float*>(smem + 4 * AMU_IMG);
    float* colw = roww + AMU_TILE;
    float* rowthr = colw + AMU_TILE;                              // (EMIT) t_row times w_a
    int* slots = reinterpret_cast<int*>(rowthr + 2 * AMU_TILE);   // (!EMIT) [slot][AMU_SLOT_STRIDE]
    const uint32_t row0 = (br0 + blockIdx.x) * AMU_TILE;
    const float ninf = -__uint_as_float(0x7F800000u);
    const uint32_t i0 = (uint32_t)((uint64_t)blockIdx.y * n_i / gridDim.y), i1 = (uint32_t)((uint64_t)(blockIdx.y + 1) * n_i / gridDim.y);

    if (tid < AMU_TILE) {
        const uint32_t r = row0 + (uint32_t)tid;
        float w = 0.0f;
        int lowest = SMY_ORD_NINF;
        if (r < n_q) {
            const uint32_t g = q_local0 + r;
            const bool dead = q_tomb && ((q_tomb[g >> 6] >> (g & 63)) & 1ull);
            if (!dead) {
                const float s = qxx[r];
                w = s < 0.0f ? -1.0f : sqrtf(s);
            }
            if (EMIT) {
                lowest = gslot[(size_t)r * m];
                for (uint32_t j = 1; j < m; ++j) lowest = min(lowest, gslot[(size_t)r * m + j]);
            }
        }
        roww[tid] = w;
        if (EMIT) rowthr[tid] = amu_unord(lowest);
    }
    if (!EMIT)
        for (int j = tid; j < AMU_SLOT_STRIDE * (int)m; j += 256) slots[j] = SMY_ORD_NINF;

    // global -> registers -> LDS: thread t moves chunk t & 7 of rows t >> 3, + 32, + 64, + 96 of both operands
    const uint16_t *ga[4], *gb[4];
    uint32_t lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (tid >> 3) + 32 * j, ch = tid & 7;
        const uint32_t ra = min(row0 + (uint32_t)row, n_q - 1);   // a ragged last tile rereads the last row
        ga[j] = qmirror + (size_t)ra * DIM + ch * 8;
        lo[j] = amu_lds_off(row, ch);
    }
    u32x4 sa[4], sb[4];
#define MI_SMY_FETCH(kc)                                                           \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                \
        sa[j] = *reinterpret_cast<const u32x4*>(ga[j] + (kc) * AMU_KC);            \
        sb[j] = *reinterpret_cast<const u32x4*>(gb[j] + (kc) * AMU_KC);            \
    }
#define MI_SMY_STASH(buf)                                                          \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                \
        *reinterpret_cast<u32x4*>(smem + (buf) * (2 * AMU_IMG) + lo[j]) = sa[j];   \
        *reinterpret_cast<u32x4*>(smem + (buf) * (2 * AMU_IMG) + AMU_IMG + lo[j]) = sb[j]; \
    }

    // operand lane map of the 32x32x16 form: lane (r = l & 31, h = l >> 5) holds elements k = 8 h .. 8 h + 7 of row r
    uint32_t fa[2], fb[2];
    const int swz_a0 = ((wr * 64 + l31) >> 1) & 7, swz_b0 = ((wc * 64 + l31) >> 1) & 7;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        fa[t] = (uint32_t)((wr * 64 + t * 32 + l31) * 128);
        fb[t] = (uint32_t)(AMU_IMG + (wc * 64 + t * 32 + l31) * 128);
    }

#pragma unroll 1
    for (uint32_t it = i0; it < i1; ++it) {
        const uint32_t col0 = (bc0 + it * step) * AMU_TILE;
        // (the previous tile's readers of the column weights and of the images passed the barrier that ends this iteration)
        if (tid < AMU_TILE) {
            const uint32_t cidx = col0 + (uint32_t)tid;
            float w = 0.0f;
            if (cidx < n_cols) {
                const bool dead = tomb && ((tomb[cidx >> 6] >> (cidx & 63)) & 1ull);
                if (!dead) {
                    const float s = xx[cidx];
                    w = s < 0.0f ? -1.0f : 1.0f / sqrtf(s);
                }
            }
            colw[tid] = w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (tid >> 3) + 32 * j, ch = tid & 7;
            const uint32_t rb = min(col0 + (uint32_t)row, n_cols - 1);
            gb[j] = mirror + (size_t)rb * DIM + ch * 8;
        }
        amu_f32x16 acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[ti][tj][e] = 0.0f;

        MI_SMY_FETCH(0)
        MI_SMY_STASH(0)
        __syncthreads();
#pragma unroll 1
        for (int kc = 0; kc < NK; ++kc) {
            if (kc + 1 < NK) { MI_SMY_FETCH(kc + 1) }
            const unsigned char* img = smem + (kc & 1) * (2 * AMU_IMG);
#pragma unroll
            for (int s = 0; s < AMU_KC / 16; ++s) {
                const int ch = 2 * s + lh;
                amu_bf16x8 af[2], bf[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    af[t] = *reinterpret_cast<const amu_bf16x8*>(img + fa[t] + ((ch ^ swz_a0) << 4));
                    bf[t] = *reinterpret_cast<const amu_bf16x8*>(img + fb[t] + ((ch ^ swz_b0) << 4));
                }
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
            }
            if (kc + 1 < NK) { MI_SMY_STASH((kc + 1) & 1) }
            __syncthreads();
        }

        // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
        const int cl0 = wc * 64 + l31, cl1 = cl0 + 32;
        const float cw0 = colw[cl0], cw1 = colw[cl1];
        if (!EMIT) {
            // the tile's columns into the slots of their residues
            int* p0 = slots + ((col0 + (uint32_t)cl0) % m) * AMU_SLOT_STRIDE + wr * 64 + 4 * lh;
            int* p1 = slots + ((col0 + (uint32_t)cl1) % m) * AMU_SLOT_STRIDE + wr * 64 + 4 * lh;
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ro = ti * 32 + 8 * q;
                    const f32x4 wa = *reinterpret_cast<const f32x4*>(roww + wr * 64 + 4 * lh + ro);
                    const amu_i32x4 mo0 = *reinterpret_cast<const amu_i32x4*>(p0 + ro);
                    const amu_i32x4 mo1 = *reinterpret_cast<const amu_i32x4*>(p1 + ro);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // (a NaN never enters a slot)
                        const int ob0 = amu_ord(fmaxf(ninf, acc[ti][0][4 * q + j] * cw0));
                        const int ob1 = amu_ord(fmaxf(ninf, acc[ti][1][4 * q + j] * cw1));
                        if (wa[j] > 0.0f && cw0 > 0.0f && ob0 > mo0[j]) atomicMax(p0 + ro + j, ob0);
                        if (wa[j] > 0.0f && cw1 > 0.0f && ob1 > mo1[j]) atomicMax(p1 + ro + j, ob1);
                    }
                }
            }
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
            const uint32_t mine = (uint32_t)__popcll(hit);
            if (__ballot(mine != 0u) != 0ull) {
                uint32_t incl = mine;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t v = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += v;
                }
                unsigned long long base = 0ull;
                if (lane == 63) base = atomicAdd(count, (unsigned long long)incl);
                base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 63, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 63, 64);
                unsigned long long at = base + incl - mine;
                while (hit) {
                    const int bit = __ffsll((long long)hit) - 1;
                    hit &= hit - 1ull;
                    const int e = bit & 15, ti = bit >> 5, tj = (bit >> 4) & 1;
                    const uint32_t a = row0 + (uint32_t)(wr * 64 + ti * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh);
                    const uint32_t b = col0 + (uint32_t)(wc * 64 + tj * 32 + l31);
                    if (at < cap) cand[at] = make_uint2(a, b);
                    ++at;
                }
            }
        }
        __syncthreads();   // the column weights and the images may be overwritten
    }
#undef MI_SMY_FETCH
#undef MI_SMY_STASH
    if (!EMIT) {
        // the segment's slots into the strip's (vector atomics on global memory; an empty slot changes nothing)
        for (int j = tid; j < AMU_TILE * (int)m; j += 256) {
            const int row = j & (AMU_TILE - 1), sl = j / AMU_TILE;
            const int v = slots[sl * AMU_SLOT_STRIDE + row];
            const uint32_t r = row0 + (uint32_t)row;
            if (r < n_q && v > SMY_ORD_NINF) atomicMax(gslot + (size_t)r * m + sl, v);
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
}  // namespace mi_assign_multi
}  // namespace mi_search_many
