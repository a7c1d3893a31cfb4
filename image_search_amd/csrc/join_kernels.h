// join_kernels.h — device code of the threshold self-join (mi_knn_near_pairs): every pair of live rows (a < b) whose cosine
// distance is <= max_dist, "which of my images are there twice?".
//
// Two stages, the contract of the two-stage search (knn_kernels.h "bf16 mirror as prefilter"): a cheap first stage that may
// only err on the side of MORE pairs, and the fp32 arithmetic of knn_scan_kernel deciding.
//
// Stage 1 (join_tiles_kernel), the matrix pipe.  S = M M^T over the bf16 mirror M (knn_mirror_kernel: rows rounded to
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
// with q = row a reports for row b, bit for bit.  Pairs with dist <= max_dist (never a NaN) are compacted as (a, b, dist).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

// knn_kernels.h defines its plain (non-template) kernels without `inline`, for the one translation unit that launches
// them.  This second one takes the shared device code (RowAcc, row16_sum, knn_mirror_kernel, IdMap) through a namespace of
// its own, so that nothing is defined twice when the library is linked and knn.hip compiles to the code it always did.
namespace mi_join {
#include "knn_kernels.h"
}

namespace mi_join {
namespace mi {

typedef __bf16 join_bf16x8 __attribute__((ext_vector_type(8)));
typedef float join_f32x16 __attribute__((ext_vector_type(16)));

constexpr int JOIN_TILE = 128;                                       // rows of a tile, both ways
constexpr int JOIN_KC = 64;                                          // elements of K per LDS image (128 bytes per row)
constexpr int JOIN_IMG = JOIN_TILE * JOIN_KC * 2;                    // bytes of one operand's image
constexpr int JOIN_LDS = 4 * JOIN_IMG + 2 * JOIN_TILE * 4;           // two buffers of two operands + the rows' weights
constexpr uint32_t JOIN_CAP_MIN = JOIN_TILE * JOIN_TILE;             // a candidate buffer holds at least one full tile
constexpr uint32_t JOIN_CAP_DEFAULT = PREF_CAP;

// 16-byte chunk `ch` (0..7) of row `row` inside an operand image of 128-byte rows.  The xor spreads the 16 rows a
// ds_read_b128 serves at once (lanes l .. l + 15: consecutive rows, one chunk) over all 64 banks: even rows start in
// banks 0..31, odd rows in 32..63, and the 8 rows of either parity take 8 different chunks.
__device__ __forceinline__ uint32_t join_lds_off(int row, int ch) { return (uint32_t)(row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)); }

// grid (column blocks, row blocks): workgroup (x, y) takes tile (bi = br0 + y, bj = bc0 + x) and leaves at once when
// bj < bi.  c = 1 - (max_dist + eps2).  count: all candidates found, also those beyond cap (the caller then redoes the
// strip in smaller pieces); cand: the first `cap` of them as (a, b) local rows.
template <int NCH>
__global__ __launch_bounds__(256) void join_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                          const uint64_t* __restrict__ tomb, uint32_t n_rows, uint32_t first_new,
                                                          uint32_t br0, uint32_t bc0, float c, uint32_t cap,
                                                          uint2* __restrict__ cand, unsigned long long* __restrict__ count) {
    static_assert(NCH % 2 == 0, "rows of whole 256-byte bf16 chunks (the mirror's own condition)");
    constexpr int DIM = NCH * 64, NK = DIM / JOIN_KC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t bi = br0 + blockIdx.y, bj = bc0 + blockIdx.x;
    if (bj < bi) return;
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const int wr = wib >> 1, wc = wib & 1, l31 = lane & 31, lh = lane >> 5;
    float* wgt = reinterpret_cast<float*>(smem + 4 * JOIN_IMG);   // [0, 128): the tile's rows a, [128, 256): its columns b
    const uint32_t row0 = bi * JOIN_TILE, col0 = bj * JOIN_TILE;

    // a row's weight: sqrt of its stored norm; -inf = marked (a candidate against everything live); NaN = not there
    {
        const bool is_col = tid >= JOIN_TILE;
        const uint32_t r = (is_col ? col0 : row0) + (uint32_t)(tid & (JOIN_TILE - 1));
        float w = __uint_as_float(0x7FC00000u);
        if (r < n_rows && !(is_col && r < first_new)) {
            const bool dead = tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull);
            if (!dead) {
                const float s = xx[r];
                w = s < 0.0f ? -__uint_as_float(0x7F800000u) : sqrtf(s);
            }
        }
        wgt[tid] = w;
    }

    // global -> registers -> LDS: thread t moves chunk t & 7 of rows t >> 3, + 32, + 64, + 96 of both operands
    const uint16_t *ga[4], *gb[4];
    uint32_t lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (tid >> 3) + 32 * j, ch = tid & 7;
        const uint32_t ra = min(row0 + (uint32_t)row, n_rows - 1), rb = min(col0 + (uint32_t)row, n_rows - 1);   // a ragged last tile rereads the last row
        ga[j] = mirror + (size_t)ra * DIM + ch * 8;
        gb[j] = mirror + (size_t)rb * DIM + ch * 8;
        lo[j] = join_lds_off(row, ch);
    }
    u32x4 sa[4], sb[4];   // (the native vector type: arrays of HIP's uint4 struct stayed in scratch memory)
#define MI_JOIN_FETCH(kc)                                                          \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                \
        sa[j] = *reinterpret_cast<const u32x4*>(ga[j] + (kc) * JOIN_KC);           \
        sb[j] = *reinterpret_cast<const u32x4*>(gb[j] + (kc) * JOIN_KC);           \
    }
#define MI_JOIN_STASH(buf)                                                         \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                \
        *reinterpret_cast<u32x4*>(smem + (buf) * (2 * JOIN_IMG) + lo[j]) = sa[j];  \
        *reinterpret_cast<u32x4*>(smem + (buf) * (2 * JOIN_IMG) + JOIN_IMG + lo[j]) = sb[j]; \
    }

    join_f32x16 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ti][tj][e] = 0.0f;

    // operand lane map of the 32x32x16 form: lane (r = l & 31, h = l >> 5) holds elements k = 8 h .. 8 h + 7 of row r
    uint32_t fa[2], fb[2];   // byte offsets of this lane's rows, chunk xor applied per read
    const int swz_a0 = ((wr * 64 + l31) >> 1) & 7, swz_b0 = ((wc * 64 + l31) >> 1) & 7;   // (+ 32 rows: the same xor, 32 >> 1 = 16)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        fa[t] = (uint32_t)((wr * 64 + t * 32 + l31) * 128);
        fb[t] = (uint32_t)(JOIN_IMG + (wc * 64 + t * 32 + l31) * 128);
    }

    MI_JOIN_FETCH(0)
    MI_JOIN_STASH(0)
    __syncthreads();
#pragma unroll 1
    for (int kc = 0; kc < NK; ++kc) {
        if (kc + 1 < NK) { MI_JOIN_FETCH(kc + 1) }
        const unsigned char* img = smem + (kc & 1) * (2 * JOIN_IMG);
#pragma unroll
        for (int s = 0; s < JOIN_KC / 16; ++s) {
            const int ch = 2 * s + lh;
            join_bf16x8 af[2], bf[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[t] = *reinterpret_cast<const join_bf16x8*>(img + fa[t] + ((ch ^ swz_a0) << 4));
                bf[t] = *reinterpret_cast<const join_bf16x8*>(img + fb[t] + ((ch ^ swz_b0) << 4));
            }
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
        }
        // the other buffer's last readers passed the barrier that ended the previous step
        if (kc + 1 < NK) { MI_JOIN_STASH((kc + 1) & 1) }
        __syncthreads();
    }
#undef MI_JOIN_FETCH
#undef MI_JOIN_STASH

    // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
    const bool diag = bi == bj;
    const float inf = __uint_as_float(0x7F800000u);
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
                const float wb = wgt[JOIN_TILE + cb];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = wa[j] * wb;
                    bool ok = p == p && (!(acc[ti][tj][4 * q + j] < c * p) || fabsf(p) == inf);
                    if (diag) ok = ok && cb > ra0 + j;
                    if (ok) hit |= 1ull << ((2 * ti + tj) * 16 + 4 * q + j);
                }
            }
        }
    }
    const uint32_t mine = (uint32_t)__popcll(hit);
    if (__ballot(mine != 0u) == 0ull) return;   // what almost every tile of a real corpus does
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
}  // namespace mi_join
