// window_kernels.h — device code of the windowed pair calls (mi_knn_near_pairs_window, mi_knn_density_window,
// mi_knn_dbscan_window): the join and the density passes over W_win, the pairs of W whose two stamps lie within `window` of
// each other (|stamp_a - stamp_b| <= window, the difference taken exactly: window_host.h).
//
// Three pieces, all in front of stage 2, which is the unwindowed calls' (join_rescore_kernel, density_count_kernel,
// density_link_kernel) and sees nothing but pairs that pass the stamp test:
//   stamp_ranges_kernel   per 128-row block the smallest and the largest stamp of its live rows (empty when it has none).
//   the tile skip         pair_tile<.., WIN = true> leaves a tile in front of its first load when the gap between the two
//                         blocks' ranges exceeds the window.  Exact: every pair of the tile is at least the gap apart.  The host
//                         decides the same from the same ranges (window_host.h) and launches only the columns of a strip
//                         where some tile survives.
//   the stamp test        the tile's 128 + 128 stamps lie in LDS behind the weights (2 KB); every element the threshold
//                         test made a candidate is dropped again unless its two stamps pass.  Candidates are rare, so the
//                         test walks the set bits of the hit mask, not the accumulators.
// No float takes part in any of it: integer compares on the stamps alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "pair_kernels.h"
#include "tile128.h"
#include "window_host.h"

namespace mi {

constexpr int WINDOW_LDS = JOIN_LDS + PAIR_WINDOW_LDS;

// one workgroup of TILE threads per 128-row block: range[block] = {min, max} of the stamps of its live rows; stamps null:
// every stamp is 0.  A block without a live row gets STAMP_RANGE_EMPTY.
static __global__ __launch_bounds__(TILE) void stamp_ranges_kernel(const int64_t* __restrict__ stamps, const uint64_t* __restrict__ tomb,
                                                                   uint32_t n_rows, StampRange* __restrict__ range) {
    __shared__ int64_t lo[TILE], hi[TILE];
    const uint32_t r = blockIdx.x * TILE + threadIdx.x;
    StampRange mine = STAMP_RANGE_EMPTY;
    if (r < n_rows && !tile_dead(tomb, r)) mine.lo = mine.hi = stamps ? stamps[r] : 0;
    lo[threadIdx.x] = mine.lo;
    hi[threadIdx.x] = mine.hi;
    __syncthreads();
#pragma unroll
    for (int d = TILE / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const int64_t l2 = lo[threadIdx.x + d], h2 = hi[threadIdx.x + d];
            if (l2 < lo[threadIdx.x]) lo[threadIdx.x] = l2;
            if (h2 > hi[threadIdx.x]) hi[threadIdx.x] = h2;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) range[blockIdx.x] = StampRange{lo[0], hi[0]};
}

// stage 1 of mi_knn_near_pairs_window and of pass 1 of the windowed density passes: join_tiles_kernel with the window
template <int NCH>
__global__ __launch_bounds__(256) void window_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                            const uint64_t* __restrict__ tomb, uint32_t n_rows, uint32_t first_new,
                                                            uint32_t br0, uint32_t bc0, float c, uint32_t cap, uint2* __restrict__ cand,
                                                            unsigned long long* __restrict__ count, PairWindow win) {
    pair_tile<NCH, true, false, true>(mirror, xx, tomb, nullptr, n_rows, mirror, xx, tomb, nullptr, n_rows, 0u, first_new, br0, bc0, c, cap,
                                      cand, count, win);
}

// stage 1 of pass 2 of mi_knn_dbscan_window: density_tiles_kernel with the window; a tile is left when either test says so
template <int NCH>
__global__ __launch_bounds__(256) void window_skip_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                                 const uint64_t* __restrict__ tomb, const uint8_t* __restrict__ act,
                                                                 uint32_t n_rows, uint32_t br0, uint32_t bc0, float c, uint32_t cap,
                                                                 uint2* __restrict__ cand, unsigned long long* __restrict__ count,
                                                                 PairWindow win) {
    pair_tile<NCH, true, true, true>(mirror, xx, tomb, act, n_rows, mirror, xx, tomb, act, n_rows, 0u, 0u, br0, bc0, c, cap, cand, count,
                                     win);
}

}  // namespace mi
