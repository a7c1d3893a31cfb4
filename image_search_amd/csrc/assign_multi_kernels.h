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
// assign_multi_finalize_kernel unpacks a strip's slots, pads behind the last hit and pads the deleted rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

// the shared device code (RowAcc, row16_sum, knn_mirror_kernel, the keys) through a namespace of its own: see join_kernels.h
namespace mi_assign_multi {
#include "knn_kernels.h"
}

namespace mi_assign_multi {
namespace mi {

typedef __bf16 amu_bf16x8 __attribute__((ext_vector_type(8)));
typedef float amu_f32x16 __attribute__((ext_vector_type(16)));
typedef int amu_i32x4 __attribute__((ext_vector_type(4)));

constexpr int AMU_TILE = 128;                                   // rows / vectors of a tile
constexpr int AMU_KC = 64;                                      // elements of K per LDS image (128 bytes per row)
constexpr int AMU_IMG = AMU_TILE * AMU_KC * 2;                  // bytes of one operand's image
constexpr int AMU_MAX_M = 16;                                   // labels per row
// two buffers of two operands + row weights, column 1 / w, column w, row thresholds + the rows' slots
constexpr int AMU_SLOT_STRIDE = AMU_TILE + 4;                   // ints between a row's slots: the 16 slots start 4 banks apart
constexpr int AMU_LDS = 4 * AMU_IMG + 4 * AMU_TILE * 4 + AMU_SLOT_STRIDE * AMU_MAX_M * 4;
constexpr uint32_t AMU_CAP_MIN = AMU_TILE * AMU_TILE;           // a candidate buffer holds at least one full tile

// the join's LDS layout (join_lds_off): 16-byte chunk `ch` of row `row`, xor-spread over the banks
__device__ __forceinline__ uint32_t amu_lds_off(int row, int ch) { return (uint32_t)(row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)); }
// floats as integers of the same order (an involution), for ds_max_i32
__device__ __forceinline__ int amu_ord(float f) { const int b = __float_as_int(f); return b ^ ((b >> 31) & 0x7FFFFFFF); }
__device__ __forceinline__ float amu_unord(int o) { return __int_as_float(o ^ ((o >> 31) & 0x7FFFFFFF)); }

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
    static_assert(NCH % 2 == 0, "rows of whole 256-byte bf16 chunks (the mirror's own condition)");
    constexpr int DIM = NCH * 64, NK = DIM / AMU_KC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const int wr = wib >> 1, wc = wib & 1, l31 = lane & 31, lh = lane >> 5;
    // weights: rows  > 0 = sqrt of the stored norm, -1 = marked, 0 = not there;  columns  colw > 0 = 1 / sqrt(norm), -1, 0
    // and colsq = sqrt(norm) where colw > 0
    float* roww = reinterpret_cast<float*>(smem + 4 * AMU_IMG);
    float* colw = roww + AMU_TILE;
    float* colsq = colw + AMU_TILE;
    float* rowthr = colsq + AMU_TILE;
    int* slots = reinterpret_cast<int*>(rowthr + AMU_TILE);   // [slot][AMU_SLOT_STRIDE]: slot j of row r at j * stride + r
    const uint32_t row0 = (br0 + blockIdx.x) * AMU_TILE;
    const float ninf = -__uint_as_float(0x7F800000u);

    if (tid < AMU_TILE) {
        const uint32_t r = row0 + (uint32_t)tid;
        float w = 0.0f;
        if (r < n_rows) {
            const bool dead = tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull);
            if (!dead) {
                const float s = xx[r];
                w = s < 0.0f ? -1.0f : sqrtf(s);
            }
        }
        roww[tid] = w;
    }
    for (int j = tid; j < AMU_SLOT_STRIDE * (int)m; j += 256) slots[j] = amu_ord(ninf);

    // global -> registers -> LDS: thread t moves chunk t & 7 of rows t >> 3, + 32, + 64, + 96 of both operands
    const uint16_t *ga[4], *gb[4];
    uint32_t lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (tid >> 3) + 32 * j, ch = tid & 7;
        const uint32_t ra = min(row0 + (uint32_t)row, n_rows - 1);   // a ragged last tile rereads the last row
        ga[j] = mirror + (size_t)ra * DIM + ch * 8;
        lo[j] = amu_lds_off(row, ch);
    }
    u32x4 sa[4], sb[4];
#define MI_AMU_FETCH(kc)                                                           \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                \
        sa[j] = *reinterpret_cast<const u32x4*>(ga[j] + (kc) * AMU_KC);            \
        sb[j] = *reinterpret_cast<const u32x4*>(gb[j] + (kc) * AMU_KC);            \
    }
#define MI_AMU_STASH(buf)                                                          \
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
    for (uint32_t bj = bc0; bj < bc1; ++bj) {
        const uint32_t col0 = bj * AMU_TILE;
        // (the previous tile's readers of the column weights and of the images passed the barrier that ends this iteration)
        if (tid < AMU_TILE) {
            const uint32_t cidx = col0 + (uint32_t)tid;
            float w = 0.0f, sq = 0.0f;
            if (cidx < n_vec) {
                const float s = vxx[cidx];
                sq = s < 0.0f ? 0.0f : sqrtf(s);
                w = s < 0.0f ? -1.0f : 1.0f / sq;
            }
            colw[tid] = w;
            colsq[tid] = sq;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (tid >> 3) + 32 * j, ch = tid & 7;
            const uint32_t rb = min(col0 + (uint32_t)row, n_vec - 1);
            gb[j] = vmirror + (size_t)rb * DIM + ch * 8;
        }
        amu_f32x16 acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[ti][tj][e] = 0.0f;

        MI_AMU_FETCH(0)
        MI_AMU_STASH(0)
        __syncthreads();
#pragma unroll 1
        for (int kc = 0; kc < NK; ++kc) {
            if (kc + 1 < NK) { MI_AMU_FETCH(kc + 1) }
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
            if (kc + 1 < NK) { MI_AMU_STASH((kc + 1) & 1) }
            __syncthreads();
        }

        // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
        const int cl0 = wc * 64 + l31, cl1 = cl0 + 32;
        const float cw0 = colw[cl0], cw1 = colw[cl1];
        // (a) the tile's columns into the slots of their residues
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
        __syncthreads();
        // t_row (times w_a): the minimum over the row's slots
        if (tid < AMU_TILE) {
            int lowest = slots[tid];
            for (uint32_t j = 1; j < m; ++j) lowest = min(lowest, slots[j * AMU_SLOT_STRIDE + tid]);
            rowthr[tid] = amu_unord(lowest);
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
        __syncthreads();   // the column weights and the images may be overwritten
    }
#undef MI_AMU_FETCH
#undef MI_AMU_STASH
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

// a strip's slots -> labels / dist of its n_local rows, [n_local][m]; MI_KNN_NO_LABEL / +inf behind a row's last hit and for
// every entry of a deleted row.  dist may be null.  *hits += the (row, label) entries written (an integer count).
__global__ __launch_bounds__(256) void assign_multi_finalize_kernel(const unsigned long long* __restrict__ slot,
                                                                    const uint64_t* __restrict__ tomb, uint32_t row_base,
                                                                    uint32_t n_local, uint32_t m, uint32_t* __restrict__ labels,
                                                                    float* __restrict__ dist, unsigned long long* __restrict__ hits) {
    const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_hit = false;
    if (at < (uint64_t)n_local * m) {
        const uint32_t r = row_base + (uint32_t)(at / m);
        const bool dead = tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull);
        const unsigned long long key = slot[at];
        uint32_t lab = MI_KNN_NO_LABEL;
        float d = __uint_as_float(0x7F800000u);
        if (!dead && key != KEY_MAX) {
            lab = (uint32_t)key;
            d = u32_to_dist((uint32_t)(key >> 32));
            is_hit = true;
        }
        labels[at] = lab;
        if (dist) dist[at] = d;
    }
    const unsigned long long b = __ballot(is_hit);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(hits, (unsigned long long)__popcll(b));
}

}  // namespace mi
}  // namespace mi_assign_multi
