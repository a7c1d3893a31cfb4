// representatives.hip — host side of mi_knn_representatives and mi_knn_representatives_stats.  The kernels and the round's
// two launches: representatives_kernels.h; the host-only rules: representatives_host.h.
//
// One call: the labels go up (or the table's group column is read where it lies); summary_prepare_kernel marks the rows that
// do not count; the k-means update's walk buckets the members (kmeans_update.h, buckets only); rep_start_kernel makes pick 0
// and the host waits once for its verdict on `start`; then the rounds are enqueued REP_CHECK_EVERY at a time, and between two
// batches the host reads one word, the picks of the batch's last round: a round without a pick means that every group is done.
// rep_reach_kernel closes; rep and rep_dist go straight into the caller's arrays, the per-group arrays through buffers of the
// call, and the picks turn into ids on the host.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "kmeans_update.h"
#include "representatives_host.h"
#include "representatives_kernels.h"
#include "scan_call.h"
#include "summary_kernels.h"
#include "two_stage.h"

using namespace mi;

extern "C" {

int mi_knn_representatives(mi_knn* t, const uint32_t* labels, uint32_t C, uint32_t m, float min_gap, const uint64_t* start, uint64_t* picks,
                           float* gap, uint32_t* n_picked, float* reach, uint32_t* rep, float* rep_dist, uint64_t totals[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = rep_check_args(t, C, m, min_gap, &why);
        if (bad != MI_OK) fail(bad, "%s (C %u, m %u)", why, C, m);
        std::lock_guard<std::mutex> l(t->mu);
        if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "not offered on a shard of a sharded table: a group's members lie on other shards");
        check_mirror_dim(t->dim, "the representatives'");
        if (t->rows >= (1ull << 32)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)t->rows);
        for (uint64_t& v : t->representatives_stats) v = 0;
        if (t->rows == 0) {
            rep_pad(C, m, picks, gap, n_picked, reach, totals);
            return;
        }
        const uint32_t n = (uint32_t)t->rows, dim = t->dim;
        const size_t cm = (size_t)C * m;
        const IdMap map = knn_id_map(t);
        const RepWindow win = rep_window(min_gap);
        std::vector<uint32_t> h_start;
        if (start) {
            h_start.resize(C);
            rep_start_rows(map, t->rows, start, C, h_start.data());
        }
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
        uint32_t* d_start_rows = nullptr;
        if (start) {
            d_start_rows = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(d_start_rows, h_start.data(), (size_t)C * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        }
        float* d_flag = (float*)scratch.get((size_t)n * sizeof(float));
        float* d_self = (float*)scratch.get((size_t)n * sizeof(float));        // summary_prepare_kernel's dist: not used here
        float* d_rep_dist = (float*)scratch.get((size_t)n * sizeof(float));
        uint32_t* d_K = (uint32_t*)scratch.get((size_t)n * sizeof(uint32_t));
        uint32_t* d_rep = (uint32_t*)scratch.get((size_t)n * sizeof(uint32_t));
        uint32_t* d_picked = (uint32_t*)scratch.get((size_t)n * sizeof(uint32_t));
        uint32_t* d_picks = (uint32_t*)scratch.get(cm * sizeof(uint32_t));
        float* d_gap = (float*)scratch.get(cm * sizeof(float));
        uint32_t* d_centre = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
        uint32_t* d_done = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
        uint32_t* d_n_picked = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
        unsigned long long* d_slots = (unsigned long long*)scratch.get((size_t)2 * C * sizeof(unsigned long long));   // the rounds', then reach
        unsigned long long* d_reach = d_slots + C;
        unsigned long long* d_read = (unsigned long long*)scratch.get((size_t)(m + 1) * sizeof(unsigned long long));
        uint32_t* d_made = (uint32_t*)scratch.get((size_t)(m + 1) * sizeof(uint32_t));
        unsigned long long* d_sw = (unsigned long long*)scratch.get(SW_WORDS * sizeof(unsigned long long));
        uint32_t* d_words = (uint32_t*)scratch.get(RW_WORDS * sizeof(uint32_t));
        KmUpdate u;
        u.alloc_buckets(scratch, n, C);
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_rep_dist, 0x7F800000, n, s));
        HIP_CHECK(hipMemsetAsync(d_K, 0xFF, (size_t)n * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(d_rep, 0xFF, (size_t)n * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(d_picked, 0, (size_t)n * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(d_picks, 0xFF, cm * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_gap, 0x7F800000, cm, s));
        HIP_CHECK(hipMemsetAsync(d_slots, 0, (size_t)2 * C * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetAsync(d_read, 0, (size_t)(m + 1) * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetAsync(d_made, 0, (size_t)(m + 1) * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(d_sw, 0, SW_WORDS * sizeof(unsigned long long), s));
        const uint32_t words0[RW_WORDS] = {0u, 0xFFFFFFFFu};
        HIP_CHECK(hipMemcpyAsync(d_words, words0, sizeof words0, hipMemcpyHostToDevice, s));
        const uint64_t* tomb = t->dead.empty() ? nullptr : t->d_tomb;
        const uint32_t grid = std::max(u.max_segs, 1u), per_group = (C + 255) / 256;
        uint32_t launched = 0;

        dispatch_nch(dim, [&](auto nch_c) {
            constexpr int NCH = decltype(nch_c)::value;
            hipLaunchKernelGGL((summary_prepare_kernel<NCH>), dim3(group16_blocks(t, n)), dim3(256), 0, s, t->table, d_labels, tomb, n, C,
                               u.d_inv, d_flag, d_self, d_sw);
            HIP_CHECK(hipGetLastError());
            u.buckets(s, d_labels, d_flag, n, C);
            hipLaunchKernelGGL(rep_start_kernel, dim3(per_group), dim3(256), 0, s, d_labels, d_flag, u.d_sorted, u.d_start, d_start_rows, n, C,
                               m, d_centre, d_done, d_n_picked, d_picks, d_picked, d_made, d_words);
            HIP_CHECK(hipGetLastError());
            if (start) {   // the one wait in front of the rounds: a start that is no member ends the call before anything is written
                uint32_t words[RW_WORDS] = {0u, 0u};
                HIP_CHECK(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                if (words[RW_BAD]) {
                    const uint32_t c = words[RW_BAD_GROUP];
                    fail(MI_ERR_INVALID, "start[%u] = %llu is not a member of group %u (%u such entries)", c, (unsigned long long)start[c], c,
                         words[RW_BAD]);
                }
            }
            for (uint32_t j = 1; j <= m;) {
                const uint32_t batch = std::min(REP_CHECK_EVERY, m - j + 1);
                for (uint32_t b = 0; b < batch; ++b, ++j, ++launched) {
                    hipLaunchKernelGGL((rep_round_kernel<NCH>), dim3(grid), dim3(256), 0, s, t->table, u.d_sorted, u.d_start, u.d_seg, C, j - 1,
                                       d_centre, d_done, d_picked, d_K, d_rep, d_slots, d_read);
                    hipLaunchKernelGGL(rep_advance_kernel, dim3(per_group), dim3(256), 0, s, C, m, j, win.key, win.bounded, d_slots, d_centre,
                                       d_done, d_n_picked, d_picks, d_gap, d_picked, d_made);
                }
                HIP_CHECK(hipGetLastError());
                if (j > m) break;
                uint32_t made = 0;   // of round j - 1: none means that every group is done
                HIP_CHECK(hipMemcpyAsync(&made, d_made + (j - 1), sizeof made, hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                if (made == 0) break;
            }
            hipLaunchKernelGGL(rep_reach_kernel, dim3(grid), dim3(256), 0, s, u.d_sorted, u.d_start, u.d_seg, C, d_K, d_rep_dist, d_reach);
            HIP_CHECK(hipGetLastError());
        });

        // the two large arrays go straight to the caller, the per-group ones through buffers of the call
        std::vector<uint32_t> h_total((size_t)C + 1), h_picks(cm), h_n((size_t)C);
        std::vector<float> h_gap(cm);
        std::vector<uint64_t> h_reach((size_t)C);
        unsigned long long last_read = 0;
        uint32_t n_segs = 0;
        HIP_CHECK(hipMemcpyAsync(h_total.data(), u.d_total, h_total.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_picks.data(), d_picks, cm * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_gap.data(), d_gap, cm * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_n.data(), d_n_picked, (size_t)C * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_reach.data(), d_reach, (size_t)C * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&last_read, d_read + launched, sizeof last_read, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&n_segs, u.d_seg + C, sizeof n_segs, hipMemcpyDeviceToHost, s));
        if (rep) HIP_CHECK(hipMemcpyAsync(rep, d_rep, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (rep_dist) HIP_CHECK(hipMemcpyAsync(rep_dist, d_rep_dist, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));

        uint64_t members = 0, sums[3] = {0, 0, 0};
        for (uint32_t c = 0; c < C; ++c) members += h_total[c];
        rep_decode(h_picks.data(), h_gap.data(), h_n.data(), h_reach.data(), C, m, map, picks, gap, n_picked, reach, sums);
        if (totals) {
            totals[0] = members; totals[1] = sums[0]; totals[2] = sums[1]; totals[3] = sums[2];
        }
        t->representatives_stats[0] = launched;
        t->representatives_stats[1] = n_segs;
        t->representatives_stats[2] = last_read;
    });
}

int mi_knn_representatives_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->representatives_stats[i];
    });
}

}  // extern "C"
