// summary.hip — host side of mi_knn_summarize and mi_knn_summarize_stats.  The kernels, the medoid identity and why the
// centroids are k-means' to the bit: summary_kernels.h; the host-only rules: summary_host.h.
//
// One call: the labels go up (or the table's group column is read where it lies); summary_prepare_kernel marks the rows that
// do not count; the update of mi_knn_kmeans (kmeans_update.h) buckets the rows and sums the centroids; summary_dist_kernel
// walks the same segments for the distances and the per-group slots; everything goes back under one wait (centroids and
// dist straight into the caller's arrays) and the slots are turned into ids on the host.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "kmeans_update.h"
#include "summary_host.h"
#include "summary_kernels.h"
#include "two_stage.h"

using namespace mi;

extern "C" {

int mi_knn_summarize(mi_knn* t, const uint32_t* labels, uint32_t C, float* centroids, uint64_t* count, uint64_t* cover, float* cover_dist,
                     uint64_t* odd, float* odd_dist, uint64_t* measured, uint64_t* spread, float* dist, uint64_t totals[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = summary_check_args(t, C, &why);
        if (bad != MI_OK) fail(bad, "%s (got %u)", why, C);
        std::lock_guard<std::mutex> l(t->mu);
        check_mirror_dim(t->dim, "the summary's");
        if (t->rows >= (1ull << 32)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)t->rows);
        for (uint64_t& v : t->summarize_stats) v = 0;
        if (t->rows == 0) {
            summary_pad(C, t->dim, centroids, count, cover, cover_dist, odd, odd_dist, measured, spread, totals);
            return;
        }
        const uint32_t n = (uint32_t)t->rows, dim = t->dim;
        Scratch scratch;
        TableCall call(t);
        hipStream_t s = call.s;
        const uint32_t* d_labels = nullptr;
        if (labels) {
            uint32_t* up = (uint32_t*)scratch.get((size_t)n * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(up, labels, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            d_labels = up;
        } else if (t->d_groups) {
            d_labels = t->d_groups;   // one id per row of capacity, MI_KNN_NO_GROUP where none was set
        } else {
            uint32_t* none = (uint32_t*)scratch.get((size_t)n * sizeof(uint32_t));
            HIP_CHECK(hipMemsetAsync(none, 0xFF, (size_t)n * sizeof(uint32_t), s));
            d_labels = none;
        }
        float* d_flag = (float*)scratch.get((size_t)n * sizeof(float));
        float* d_dist = (float*)scratch.get((size_t)n * sizeof(float));
        float* d_cent = (float*)scratch.get((size_t)C * dim * sizeof(float));
        unsigned long long* d_slots = (unsigned long long*)scratch.get((size_t)SUMMARY_PLANES * C * sizeof(unsigned long long));
        unsigned long long* d_words = (unsigned long long*)scratch.get(SW_WORDS * sizeof(unsigned long long));
        KmUpdate u;
        u.alloc(scratch, n, C, dim, t->kmeans_fixed_sum != 0);
        HIP_CHECK(hipMemsetAsync(d_cent, 0, (size_t)C * dim * sizeof(float), s));   // (the update leaves an empty group's alone)
        HIP_CHECK(hipMemsetAsync(d_slots, 0xFF, (size_t)C * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetAsync(d_slots + C, 0, (size_t)(SUMMARY_PLANES - 1) * C * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetAsync(d_words, 0, SW_WORDS * sizeof(unsigned long long), s));
        const uint64_t* tomb = t->dead.empty() ? nullptr : t->d_tomb;
        const uint32_t grid = std::max(u.max_segs, 1u);
        dispatch_nch(dim, [&](auto nch_c) {
            constexpr int NCH = decltype(nch_c)::value;
            hipLaunchKernelGGL((summary_prepare_kernel<NCH>), dim3(group16_blocks(t, n)), dim3(256), 0, s, t->table, d_labels, tomb, n, C,
                               u.d_inv, d_flag, d_dist, d_words);
            HIP_CHECK(hipGetLastError());
            u.run<NCH>(t, s, d_labels, d_flag, n, C, d_cent);
            hipLaunchKernelGGL((summary_dist_kernel<NCH>), dim3(grid), dim3(256), 0, s, t->table, d_cent, u.d_sorted, u.d_start, u.d_seg, C,
                               d_dist, d_slots);
            HIP_CHECK(hipGetLastError());
        });

        // the two large arrays go straight to the caller (as mi_knn_kmeans' do), the small ones through buffers of the call
        std::vector<uint32_t> h_total((size_t)C + 1);
        std::vector<uint64_t> h_slots((size_t)SUMMARY_PLANES * C);
        unsigned long long words[SW_WORDS] = {0, 0};
        uint32_t n_segs = 0;
        HIP_CHECK(hipMemcpyAsync(h_total.data(), u.d_total, h_total.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_slots.data(), d_slots, h_slots.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&n_segs, u.d_seg + C, sizeof n_segs, hipMemcpyDeviceToHost, s));
        if (centroids) HIP_CHECK(hipMemcpyAsync(centroids, d_cent, (size_t)C * dim * sizeof(float), hipMemcpyDeviceToHost, s));
        if (dist) HIP_CHECK(hipMemcpyAsync(dist, d_dist, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));

        uint64_t members = 0, groups = 0;
        for (uint32_t c = 0; c < C; ++c) {
            members += h_total[c];
            groups += h_total[c] != 0;
            if (count) count[c] = h_total[c];
        }
        summary_decode(h_slots.data(), h_total.data(), C, knn_id_map(t), cover, cover_dist, odd, odd_dist, measured, spread);
        if (totals) {
            totals[0] = members; totals[1] = words[SW_OUTSIDE]; totals[2] = words[SW_UNUSABLE]; totals[3] = groups;
        }
        t->summarize_stats[0] = n_segs;
        t->summarize_stats[1] = grid;
        t->summarize_stats[2] = members;
    });
}

int mi_knn_summarize_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->summarize_stats[i];
    });
}

}  // extern "C"
