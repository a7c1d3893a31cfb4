// kmeans_update.h — the bucket-and-sum sequence behind the update step of mi_knn_kmeans (assign.hip) and behind the
// centroids of mi_knn_summarize (summary.hip): one set of launches, so that both calls sum in the same order and leave the
// same bits.  The kernels and the order they fix: assign_kernels.h ("the update of mi_knn_kmeans").  With `fixed` (option
// "kmeans_fixed_sum"; mi_knn_sharded_kmeans always) the same buckets are summed as exact integers of 2^-30, which no order
// changes: that form can be added across shards (kmeans_sharded.hip).
#pragma once
#include <algorithm>

#include "assign_kernels.h"
#include "common.h"
#include "handles.h"
#include "two_stage.h"

namespace mi {

// one update: labels / dist -> centroids, in an order the row ids fix.  A row feeds the centroid of its label unless the
// label is >= C or its dist is NaN (km_bucket); an empty cluster's centroid is left as it is.
struct KmUpdate {
    uint32_t n_waves = 0, chunk = 0, max_segs = 0;
    uint32_t *d_hist = nullptr, *d_total = nullptr, *d_start = nullptr, *d_seg = nullptr, *d_sorted = nullptr;
    float *d_inv = nullptr, *d_part = nullptr;
    bool fixed = false;
    long long *d_ipart = nullptr, *d_S = nullptr;   // fixed: the segments' sums [max_segs][dim], the clusters' [C][dim]
    uint32_t* d_n = nullptr;                        // ... and the clusters' sizes [C]

    // the buffers for n rows and C clusters; d_inv [n] is the caller's to fill (inv_norms, or a pass of its own that
    // leaves the same values)
    void alloc(Scratch& scratch, uint32_t n, uint32_t C, uint32_t dim, bool fixed_sum = false) {
        fixed = fixed_sum;
        alloc_buckets(scratch, n, C);
        if (!fixed) {
            d_part = (float*)scratch.get((size_t)max_segs * dim * sizeof(float));
        } else {
            d_ipart = (long long*)scratch.get((size_t)max_segs * dim * sizeof(long long));
            d_S = (long long*)scratch.get((size_t)C * dim * sizeof(long long));
            d_n = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
        }
    }

    // what buckets() alone needs (a call that walks the segments without summing them: mi_knn_representatives), and d_inv
    void alloc_buckets(Scratch& scratch, uint32_t n, uint32_t C) {
        n_waves = std::max<uint32_t>(1u, std::min<uint32_t>({4096u, (1u << 24) / (C + 1), (n + 1023) / 1024}));
        n_waves = (n_waves + 3) / 4 * 4;
        chunk = ((n + n_waves - 1) / n_waves + 63) / 64 * 64;
        max_segs = n / KM_SEG + C;
        d_hist = (uint32_t*)scratch.get((size_t)n_waves * (C + 1) * sizeof(uint32_t));
        d_total = (uint32_t*)scratch.get((size_t)(C + 2) * sizeof(uint32_t));
        d_start = (uint32_t*)scratch.get((size_t)(C + 2) * sizeof(uint32_t));
        d_seg = (uint32_t*)scratch.get((size_t)(C + 2) * sizeof(uint32_t));
        d_sorted = (uint32_t*)scratch.get((size_t)n * sizeof(uint32_t));
        d_inv = (float*)scratch.get((size_t)n * sizeof(float));
    }

    template <int NCH>
    void inv_norms(const mi_knn* t, hipStream_t s, uint32_t n) {
        hipLaunchKernelGGL((km_inv_norm_kernel<NCH>), dim3(group16_blocks(t, n)), dim3(256), 0, s, t->table, n, d_inv);
        HIP_CHECK(hipGetLastError());
    }

    // labels / dist -> the rows bucketed by label, stably: d_total, d_start, d_seg, d_sorted
    void buckets(hipStream_t s, const uint32_t* d_labels, const float* d_dist, uint32_t n, uint32_t C) {
        HIP_CHECK(hipMemsetAsync(d_hist, 0, (size_t)n_waves * (C + 1) * sizeof(uint32_t), s));
        hipLaunchKernelGGL(km_hist_kernel, dim3(n_waves / 4), dim3(256), 0, s, d_labels, d_dist, n, C, chunk, d_hist);
        hipLaunchKernelGGL(km_scan_kernel, dim3((C + 1 + 255) / 256), dim3(256), 0, s, d_hist, n_waves, C, d_total);
        hipLaunchKernelGGL(km_offsets_kernel, dim3(1), dim3(1024), 0, s, d_total, C, d_start, d_seg);
        hipLaunchKernelGGL(km_place_kernel, dim3(n_waves / 4), dim3(256), 0, s, d_labels, d_dist, n, C, chunk, d_hist, d_start, d_sorted);
    }

    // fixed: the buckets and their integer sums -> d_S [C][dim], d_n [C]
    template <int NCH>
    void sums_fixed(const mi_knn* t, hipStream_t s, const uint32_t* d_labels, const float* d_dist, uint32_t n, uint32_t C) {
        buckets(s, d_labels, d_dist, n, C);
        hipLaunchKernelGGL((km_sum_fixed_kernel<NCH>), dim3(std::max(max_segs, 1u)), dim3(256), 0, s, t->table, d_inv, d_sorted, d_start,
                           d_seg, C, d_ipart);
        const uint64_t el = (uint64_t)C * t->dim;
        hipLaunchKernelGGL(km_reduce_fixed_kernel, dim3((uint32_t)((el + 255) / 256)), dim3(256), 0, s, d_ipart, d_total, d_seg, C, t->dim,
                           d_S, d_n);
        HIP_CHECK(hipGetLastError());
    }

    // sums and sizes (one shard's, or all shards' merged) -> centroids
    static void centroids_fixed(hipStream_t s, const long long* S, const uint32_t* cnt, uint32_t C, uint32_t dim, float* d_vec) {
        const uint64_t el = (uint64_t)C * dim;
        hipLaunchKernelGGL(km_centroid_fixed_kernel, dim3((uint32_t)((el + 255) / 256)), dim3(256), 0, s, S, cnt, C, dim, d_vec);
        HIP_CHECK(hipGetLastError());
    }

    template <int NCH>
    void run(const mi_knn* t, hipStream_t s, const uint32_t* d_labels, const float* d_dist, uint32_t n, uint32_t C, float* d_vec) {
        if (fixed) {
            sums_fixed<NCH>(t, s, d_labels, d_dist, n, C);
            centroids_fixed(s, d_S, d_n, C, t->dim, d_vec);
            return;
        }
        buckets(s, d_labels, d_dist, n, C);
        hipLaunchKernelGGL((km_sum_kernel<NCH>), dim3(std::max(max_segs, 1u)), dim3(256), 0, s, t->table, d_inv, d_sorted, d_start, d_seg,
                           C, d_part);
        const uint64_t el = (uint64_t)C * t->dim;
        hipLaunchKernelGGL(km_centroid_kernel, dim3((uint32_t)((el + 255) / 256)), dim3(256), 0, s, d_part, d_total, d_seg, C, t->dim,
                           d_vec);
        HIP_CHECK(hipGetLastError());
    }
};

}  // namespace mi
