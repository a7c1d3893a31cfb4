// pair_kernels.h — the two pieces of device code every threshold-pair call shares (the join, the join of two row sets, the
// density passes on one table, at several levels and across shards, and the diverse search's conflict pass):
//     pair_tile   stage 1: one 128 x 128 tile of S = M_a M_b^T (tile128.h) -> the candidate pairs of the tile,
//     pair_dist   stage 2: the exact distance of one candidate pair, in mi_knn_search's arithmetic.
// The bound eps2 that makes stage 1 a superset of the pairs within max_dist is derived in join_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "tile128.h"
#include "window_host.h"

namespace mi {

constexpr int JOIN_LDS = TILE_IMGS + 2 * TILE * 4;                   // the tile's images + the rows' weights
constexpr int PAIR_WINDOW_LDS = 2 * TILE * 8;                        // WIN: the rows' stamps behind them

// WIN: what the windowed calls add (window_kernels.h).  stamps: one per row, null = every stamp is 0; range: one per 128-row
// block (stamp_ranges_kernel).  Both sides of a tile read the same two arrays: the windowed calls are self passes.
struct PairWindow {
    const int64_t* stamps;
    const StampRange* range;
    uint64_t window;
};

// Tile (bi = br0 + blockIdx.y, bj = bc0 + blockIdx.x) of the rows of A against the rows of B; all 256 threads of the
// workgroup call it with JOIN_LDS bytes of dynamic LDS.  c = 1 - (max_dist + eps2): element (ra, cb) is a candidate when
// !(acc < c * sqrt(xx_a) * sqrt(xx_b)); a row the mirror marked (weight -inf) is one against everything live, a row that
// is deleted or beyond its table (weight NaN) never.  count: all candidates found, also those beyond cap (the caller then
// redoes the rectangle in smaller pieces); cand: the first `cap` of them as (ra, cb) local rows.
//   SELF: A and B are one table (the caller passes its one mirror, xx and tomb as both sides).  Only tiles on or above
//         the diagonal are computed, a diagonal tile keeps cb > ra, and fn_b is the join's first_new: a column below it
//         is not there.  fn_a is not read.
//   else: every tile, every element; (fn_a, fn_b): element (ra, cb) can be a candidate only if ra >= fn_a or cb >= fn_b
//         (the host launches no tile that lies wholly below both bounds; 0, 0: everything).
//   SKIP: the density passes' test in front of the first load.  act_a[bi], act_b[bj]: bit 0 = some row of the block has a
//         neighbour within, bit 1 = some row is a core; the tile is left at once unless both blocks have bit 0 and one has
//         bit 1.  Without SKIP the two arrays are not read.
//   WIN:  the stamp test of the windowed calls, with PAIR_WINDOW_LDS more bytes of LDS.  The tile is left at once when the gap
//         between the two blocks' stamp ranges exceeds win.window, and an element is a candidate only if its two stamps lie
//         within win.window of each other (window_host.h: stamp_within; a marked row takes the test like any other).
//         Without WIN `win` is not read and the tile is what it was before the parameter existed.
template <int NCH, bool SELF, bool SKIP, bool WIN = false>
__device__ __forceinline__ void pair_tile(const uint16_t* __restrict__ mirror_a, const float* __restrict__ xx_a,
                                          const uint64_t* __restrict__ tomb_a, const uint8_t* __restrict__ act_a, uint32_t n_a,
                                          const uint16_t* __restrict__ mirror_b, const float* __restrict__ xx_b,
                                          const uint64_t* __restrict__ tomb_b, const uint8_t* __restrict__ act_b, uint32_t n_b,
                                          uint32_t fn_a, uint32_t fn_b, uint32_t br0, uint32_t bc0, float c, uint32_t cap,
                                          uint2* __restrict__ cand, unsigned long long* __restrict__ count,
                                          PairWindow win = PairWindow{nullptr, nullptr, 0}) {
    constexpr int DIM = NCH * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t bi = br0 + blockIdx.y, bj = bc0 + blockIdx.x;
    if constexpr (SELF) {
        if (bj < bi) return;
    }
    if constexpr (WIN) {
        if (!window_tile_live(win.range[bi], win.range[bj], win.window)) return;   // no pair within the window lies in this tile
    }
    if constexpr (SKIP) {
        const uint32_t fa = act_a[bi], fb = act_b[bj];
        if (!((fa & fb & 1u) && ((fa | fb) & 2u))) return;   // no pair with a core end lies in this tile
    }
    const int tid = threadIdx.x;
    const TileFrag f = tile_frag();
    const int wr = f.wr, wc = f.wc, l31 = f.l31, lh = f.lh;
    float* wgt = reinterpret_cast<float*>(smem + TILE_IMGS);   // [0, 128): the tile's rows of A, [128, 256): its rows of B
    const uint32_t row0 = bi * TILE, col0 = bj * TILE;
    const float inf = __uint_as_float(0x7F800000u);

    // a row's weight: sqrt of its stored norm; -inf = marked (a candidate against everything live); NaN = not there
    {
        const bool is_col = tid >= TILE;
        const uint32_t r = (is_col ? col0 : row0) + (uint32_t)(tid & (TILE - 1));
        bool there = r < (is_col ? n_b : n_a);
        if constexpr (SELF) there = there && !(is_col && r < fn_b);
        wgt[tid] = tile_weight<false>(is_col ? xx_b : xx_a, r, there, is_col ? tomb_b : tomb_a, r, -inf, __uint_as_float(0x7FC00000u));
        if constexpr (WIN) {
            int64_t* stamp = reinterpret_cast<int64_t*>(smem + JOIN_LDS);   // [0, 128): the rows' stamps, [128, 256): the columns'
            stamp[tid] = (win.stamps && r < (is_col ? n_b : n_a)) ? win.stamps[r] : 0;
        }
    }

    const uint16_t *ga[4], *gb[4];
    tile_src<DIM>(ga, mirror_a, row0, n_a);
    tile_src<DIM>(gb, mirror_b, col0, n_b);
    f32x16 acc[2][2];
    tile_accumulate<NCH>(smem, f, ga, gb, acc);

    // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block.
    // A cross tile that straddles a bound: rows below fn_a pair only with columns >= fn_b.  `rlo` = the tile rows below fn_a
    // (0 when the whole tile qualifies by its rows or by its columns: then the test below never fires).
    const bool diag = bi == bj;
    const uint32_t rlo = (SELF || col0 >= fn_b || row0 >= fn_a) ? 0u : min(fn_a - row0, (uint32_t)TILE);
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
                const bool col_new = SELF || col0 + (uint32_t)cb >= fn_b;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = wa[j] * wb;
                    bool ok = p == p && (!(acc[ti][tj][4 * q + j] < c * p) || fabsf(p) == inf);
                    if constexpr (SELF) {
                        if (diag) ok = ok && cb > ra0 + j;
                    } else {
                        ok = ok && (col_new || (uint32_t)(ra0 + j) >= rlo);
                    }
                    if (ok) hit |= 1ull << ((2 * ti + tj) * 16 + 4 * q + j);
                }
            }
        }
    }
    if constexpr (WIN) {
        // candidates are rare: the stamp test walks the set bits (tile_append's decoding of them), not the accumulators
        const int64_t* stamp = reinterpret_cast<const int64_t*>(smem + JOIN_LDS);
        for (unsigned long long h = hit; h;) {
            const int bit = __ffsll((long long)h) - 1;
            h &= h - 1ull;
            const int e = bit & 15, ti = bit >> 5, tj = (bit >> 4) & 1;
            const int ra = wr * 64 + ti * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh, cb = wc * 64 + tj * 32 + l31;
            if (!stamp_within(stamp[ra], stamp[TILE + cb], win.window)) hit &= ~(1ull << bit);
        }
    }
    tile_append(hit, f, row0, col0, cap, cand, count);
}

// The distance of row x from the query row q, 1 - q.x / (|q| |x|), as mi_knn_search reports it, bit for bit: sqrt(q.q)
// from RowAcc in a row's summation order (knn_scan_kernel / knn_rescore_kernel), the row streamed once for the dot product
// and its own norm.  All 16 lanes of a group call it with their i = lane & 15; every lane gets the value.  (The two roles
// round differently: which row of a pair is the query is the caller's rule.)  The density kernels call it; join_rescore_kernel,
// cross_rescore_kernel and diverse_rescore_kernel hold the same lines written out, because as a call the block compiles to
// another register allocation there at NCH >= 8 (66 -> 126 VGPRs in join_rescore_kernel<12>): change both together.
template <int NCH>
__device__ __forceinline__ float pair_dist(const float* __restrict__ q, const float* __restrict__ x, int i) {
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

}  // namespace mi
