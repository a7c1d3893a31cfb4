// where_kernels.h — a predicate over the table's side columns turned into the ascending list of qualifying local rows, the
// form the gathered search (knn_scan_gather_kernel over t->d_flist) reads.  An ordered two-pass compaction, integers only:
//
//   where_count_kernel    a workgroup owns one contiguous chunk of rows (option "where_chunk", a multiple of 64), its four
//                         waves a contiguous quarter of the chunk's 64-row tiles each.  Lane L of a wave reads row
//                         chunk_base + 64 j + L: every column load is one contiguous run of 64 words.  A wave's count is the
//                         sum of popcount(ballot) over its tiles; the chunk writes ONE count.
//   where_offsets_kernel  one workgroup turns the chunk counts into exclusive offsets, in place, 1024 at a time with a
//                         carry, and leaves the total in a 64-bit word the host copies to pinned memory.
//   where_emit_kernel     the count pass's chunking and predicate again.  A tile's ballot goes to LDS and into the wave's
//                         count; the waves' bases are the sums of the lower waves' counts, through LDS; then every tile's
//                         set lanes write their row at offsets[chunk] + wave base + the tiles before + popcount(lower lanes).
//
// No workgroup ever waits for another one: the ordering between the passes is the stream's.  The list ascends by
// construction (chunks, waves within a chunk, tiles within a wave and lanes within a tile all ascend and own contiguous
// rows), which the selection behind it relies on: knn_select_keys32 orders by (distance, position).  Nothing depends on the
// grid: the same rows for any "where_chunk".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "where_pred.h"   // WherePred, pred_of, where_match: the row test

namespace mi {

constexpr int WHERE_THREADS = 256, WHERE_WAVES = WHERE_THREADS / 64;
constexpr int WHERE_SCAN_THREADS = 1024;
constexpr uint32_t WHERE_TILES_MAX = 1024;   // tiles of the largest chunk (65536 rows): the emit pass keeps a ballot per tile in LDS

// the tiles [first, last) of the chunk's `tiles` that wave `w` owns: a contiguous quarter, the last ones possibly empty
__device__ __forceinline__ void where_wave_tiles(uint32_t tiles, uint32_t w, uint32_t* first, uint32_t* last) {
    const uint32_t per = (tiles + WHERE_WAVES - 1) / WHERE_WAVES;
    *first = min(w * per, tiles);
    *last = min(*first + per, tiles);
}

// counts [chunks]: the qualifying rows of chunk blockIdx.x.  chunk = rows per workgroup, a multiple of 64
__global__ void __launch_bounds__(WHERE_THREADS) where_count_kernel(WherePred p, const unsigned long long* __restrict__ tags,
                                                                    const long long* __restrict__ stamps,
                                                                    const uint32_t* __restrict__ groups,
                                                                    const unsigned long long* __restrict__ tomb, uint64_t rows,
                                                                    uint32_t chunk, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_cnt[WHERE_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * chunk;
    uint32_t first, last;
    where_wave_tiles(chunk / 64, w, &first, &last);
    uint32_t cnt = 0;
    for (uint32_t j = first; j < last; ++j) {
        const uint64_t row = base + (uint64_t)j * 64 + lane;
        cnt += (uint32_t)__popcll(__ballot(where_match(p, tags, stamps, groups, tomb, row, rows)));
    }
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int i = 0; i < WHERE_WAVES; ++i) sum += wave_cnt[i];
        counts[blockIdx.x] = sum;
    }
}

// counts [n] -> their exclusive prefix sums, in place; *total = the sum.  One workgroup; WHERE_SCAN_THREADS counts a round
__global__ void __launch_bounds__(WHERE_SCAN_THREADS) where_offsets_kernel(uint32_t* __restrict__ counts, uint32_t n,
                                                                           unsigned long long* __restrict__ total) {
    constexpr int WAVES = WHERE_SCAN_THREADS / 64;
    __shared__ uint32_t wave_sum[WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long carry = 0;   // the sum of the rounds before: the same value in every thread
    for (uint32_t i0 = 0; i0 < n; i0 += WHERE_SCAN_THREADS) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < n ? counts[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[w] = incl;
        __syncthreads();
        uint32_t below = 0, round = 0;
#pragma unroll
        for (int x = 0; x < WAVES; ++x) {
            const uint32_t s = wave_sum[x];
            below += x < (int)w ? s : 0u;
            round += s;
        }
        // a list holds fewer than 2^32 rows (a shard's limit): the offsets fit their 32-bit words
        if (i < n) counts[i] = (uint32_t)(carry + below + incl - v);
        carry += round;
        __syncthreads();   // wave_sum is rewritten by the next round
    }
    if (threadIdx.x == 0) *total = carry;
}

// list [offsets[chunk] ...): the qualifying rows of chunk blockIdx.x, ascending.  offsets = where_offsets_kernel's output over
// where_count_kernel's counts for the same arguments
__global__ void __launch_bounds__(WHERE_THREADS) where_emit_kernel(WherePred p, const unsigned long long* __restrict__ tags,
                                                                   const long long* __restrict__ stamps,
                                                                   const uint32_t* __restrict__ groups,
                                                                   const unsigned long long* __restrict__ tomb, uint64_t rows,
                                                                   uint32_t chunk, const uint32_t* __restrict__ offsets,
                                                                   uint32_t* __restrict__ list) {
    __shared__ unsigned long long mask_of[WHERE_TILES_MAX];
    __shared__ uint32_t wave_cnt[WHERE_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * chunk;
    uint32_t first, last;
    where_wave_tiles(chunk / 64, w, &first, &last);
    uint32_t cnt = 0;
    for (uint32_t j = first; j < last; ++j) {
        const uint64_t row = base + (uint64_t)j * 64 + lane;
        const unsigned long long m = __ballot(where_match(p, tags, stamps, groups, tomb, row, rows));
        if (lane == 0) mask_of[j] = m;
        cnt += (uint32_t)__popcll(m);
    }
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    uint64_t at = offsets[blockIdx.x];
    for (uint32_t x = 0; x < w; ++x) at += wave_cnt[x];
    for (uint32_t j = first; j < last; ++j) {
        const unsigned long long m = mask_of[j];   // written by this wave's lane 0, read behind the barrier
        if ((m >> lane) & 1ull) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            list[at + rank] = (uint32_t)(base + (uint64_t)j * 64 + lane);
        }
        at += (uint32_t)__popcll(m);
    }
}

}  // namespace mi
