// summary_kernels.h — device code of mi_knn_summarize: per group of rows its centroid, its cover (the member nearest to the
// centroid), its odd one out (the farthest), how many members were measured and the sum of their distances.
//
// Why the cover means something.  For unit vectors  sum_j (1 - x_i . x_j) = n - x_i . S  with S = sum_j x_j, so the member with
// the largest cosine to S — the member nearest to the centroid S / n — is the one with the smallest total cosine distance to
// the other members: the group's exact medoid, found without the n^2 pairs.  (In real arithmetic; the device rounds, and what
// it reports are the search's distance bits against the centroid.)
//
// The centroid comes from the update step of mi_knn_kmeans, launch for launch (kmeans_update.h): the rows bucketed by label
// with the stable counting sort, segments of KM_SEG members, the four waves of a segment combined as (0 + 1) + (2 + 3), the
// segments added in order — so a summary of k-means' own labels returns k-means' centroids to the bit.  What the sort needs
// beside the labels is one float per row that is NaN where the row must not count; summary_prepare_kernel writes it.
//
// summary_dist_kernel then walks the same segments: one workgroup per segment, the group's centroid in registers, each member
// row read once, its distance to the centroid in the arithmetic of assign_rescore_kernel (the row is the query, the centroid
// the streamed vector: dist = 1 - dot / (sqrt(q.q) * sqrt(c.c)), summed as RowAcc sums), then ONE atomicMin, one atomicMax and
// two atomicAdd per workgroup into the group's 64-bit slots (summary_host.h).  All four are integer operations whose result
// does not depend on the order of arrival; there is no float atomic and no per-row atomic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assign_kernels.h"
#include "knn_shared.h"
#include "summary_host.h"

namespace mi {

// counters of summary_prepare_kernel
constexpr int SW_OUTSIDE = 0, SW_UNUSABLE = 1, SW_WORDS = 2;

// One pass over every row, a 16-lane group per row:
//   inv[r]   1 / |x|, the norm summed as the scan sums it (km_inv_norm_kernel's value)
//   usable   the row's distance to itself in the search's arithmetic is a number (kmpp_pass_kernel<NCH, true>'s test)
//   flag[r]  NaN for a deleted or unusable row, else 0: the "dist" km_bucket reads
//   dist[r]  NaN for a live unusable row with a label < C, else +inf (summary_dist_kernel overwrites the members')
//   words    += {live rows with a label >= C, live unusable rows with a label < C}, one atomicAdd each per workgroup
template <int NCH>
__global__ __launch_bounds__(256) void summary_prepare_kernel(const float* __restrict__ table, const uint32_t* __restrict__ labels,
                                                              const uint64_t* __restrict__ tomb, uint32_t n_rows, uint32_t C,
                                                              float* __restrict__ inv, float* __restrict__ flag, float* __restrict__ dist,
                                                              unsigned long long* __restrict__ words) {
    constexpr int DIM = NCH * 64;
    __shared__ uint32_t part[16][2];
    const int lane = threadIdx.x & 63, i = lane & 15, g = threadIdx.x >> 4;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    uint32_t outside = 0, unusable = 0;
    // (whole waves stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t r0 = group; r0 < ((n_rows + n_groups - 1) / n_groups) * n_groups; r0 += n_groups) {
        const bool there = r0 < n_rows;
        const uint32_t r = there ? r0 : n_rows - 1;
        const f32x4* p = reinterpret_cast<const f32x4*>(table + (uint64_t)r * DIM) + i;
        f32x4 qf[NCH];
#pragma unroll
        for (int t = 0; t < NCH; ++t) qf[t] = p[16 * t];
        float xx, sq;
        {
            RowAcc<NCH> a; a.zero();
#pragma unroll
            for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
            xx = a.sumsq();
            sq = sqrtf(xx);
        }
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
        const float d = a.dot(), s = a.sumsq();
        const float self = 1.0f - d / (sq * sqrtf(s));
        if (there && i == 0) {
            const bool dead = tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull);
            const bool usable = self == self, in = labels[r] < C;
            inv[r] = 1.0f / sqrtf(xx);
            flag[r] = (dead || !usable) ? __uint_as_float(0x7FC00000u) : 0.0f;
            dist[r] = (!dead && in && !usable) ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
            outside += (!dead && !in) ? 1u : 0u;
            unusable += (!dead && in && !usable) ? 1u : 0u;
        }
    }
    if (i == 0) { part[g][0] = outside; part[g][1] = unusable; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long all = 0ull;
        for (int u = 0; u < 16; ++u) all += part[u][threadIdx.x];
        if (all) atomicAdd(words + threadIdx.x, all);
    }
}

// workgroup g = segment g of km_sum_kernel (of group c: seg[c] <= g < seg[c + 1]): dist[r] of its members, and the group's
// slots (four planes of C words: summary_host.h)
template <int NCH>
__global__ __launch_bounds__(256) void summary_dist_kernel(const float* __restrict__ table, const float* __restrict__ centroids,
                                                           const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ start,
                                                           const uint32_t* __restrict__ seg, uint32_t C, float* __restrict__ dist,
                                                           unsigned long long* __restrict__ slots) {
    constexpr int DIM = NCH * 64;
    __shared__ unsigned long long red[4][SUMMARY_PLANES];
    const uint32_t g = blockIdx.x;
    if (g >= seg[C]) return;
    uint32_t lo = 0, hi = C;   // the last c with seg[c] <= g
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t first = start[c] + (g - seg[c]) * KM_SEG;
    const uint32_t n = min((uint32_t)KM_SEG, start[c + 1] - first);
    const int lane = threadIdx.x & 63, i = lane & 15, grp = threadIdx.x >> 4, wib = threadIdx.x >> 6;
    // lane i of a 16-lane group holds elements 64 t + 4 i .. + 3 of the centroid
    f32x4 cf[NCH];
    {
        const f32x4* pc = reinterpret_cast<const f32x4*>(centroids + (uint64_t)c * DIM) + i;
#pragma unroll
        for (int t = 0; t < NCH; ++t) cf[t] = pc[16 * t];
    }
    float cs;   // sqrt(c.c), summed as a streamed row's
    {
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(cf[t], cf[t]);
        cs = sqrtf(a.sumsq());
    }
    unsigned long long mn = SUMMARY_MIN_INIT, mx = SUMMARY_MAX_INIT, cnt = 0ull, sum = 0ull;
    // (whole waves stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t m0 = 0; m0 < n; m0 += 16) {
        const uint32_t m = m0 + (uint32_t)grp;
        const bool live = m < n;
        const uint32_t r = sorted[first + (live ? m : 0u)];
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)r * DIM) + i;
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
        for (int t = 0; t < NCH; ++t) a.step(qf[t], cf[t]);
        const float d = a.dot();
        const float dd = 1.0f - d / (sq * cs);
        if (live && i == 0) {
            dist[r] = dd;
            const uint32_t key = dist_to_u32(dd);
            mn = umin64(mn, summary_min_word(key, r));
            if (dd == dd) {
                mx = umax64(mx, summary_max_word(key, r));
                cnt += 1ull;
                sum += summary_weight(dd);
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        mn = umin64(mn, shfl_xor64(mn, off));
        mx = umax64(mx, shfl_xor64(mx, off));
        cnt += shfl_xor64(cnt, off);
        sum += shfl_xor64(sum, off);
    }
    if (lane == 0) { red[wib][0] = mn; red[wib][1] = mx; red[wib][2] = cnt; red[wib][3] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = umin64(mn, red[w][0]);
            mx = umax64(mx, red[w][1]);
            cnt += red[w][2];
            sum += red[w][3];
        }
        atomicMin(slots + c, mn);
        atomicMax(slots + (size_t)C + c, mx);
        atomicAdd(slots + (size_t)2 * C + c, cnt);
        atomicAdd(slots + (size_t)3 * C + c, sum);
    }
}

}  // namespace mi
