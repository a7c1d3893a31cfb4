// summary_sharded.hip — host side of mi_knn_sharded_summarize and mi_knn_sharded_summarize_stats: mi_knn_summarize over a
// block-cyclic table.  Every shard marks its rows (summary_prepare_kernel), sums its members per group as exact integers of
// 2^-30 (kmeans_update.h) and, once the merged centroids are back (kmeans_sharded_merge.h, the exchange of
// mi_knn_sharded_kmeans), measures its members against them (summary_dist_kernel); its per-group slots then go from local rows
// to global ids and are folded into shard 0's (summary_sharded_kernels.h).  Integer sums, minima and maxima are the same in
// any order, so the result is the single table's with "kmeans_fixed_sum" = 1, bit for bit, whatever the layout.  The rules
// without HIP in them: summary_sharded_host.h, summary_host.h, kmeans_fixed_host.h.
//
// Streams: a shard's work runs on its own stream, behind every write and search enqueued on the shard before the call.  Shard
// 0's stream waits for the event behind every other shard's sums and, later, slots; every other shard's stream waits for the
// event behind the centroids.  The host waits once per shard, for the results.
#include <algorithm>
#include <cstring>

#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "density_sharded_host.h"   // scatter_to_global
#include "handles.h"
#include "kmeans_fixed_host.h"
#include "kmeans_sharded_merge.h"
#include "kmeans_update.h"
#include "sharded_call.h"
#include "summary_host.h"
#include "summary_kernels.h"
#include "summary_sharded_host.h"
#include "summary_sharded_kernels.h"
#include "two_stage.h"

using namespace mi;

namespace {

// one shard's state for the call; its device memory lives in `scratch`, on the shard's device
struct SumShard : KmPart {
    Scratch scratch;
    KmUpdate u;
    IdMap map{0, 0, 0, 0};
    uint32_t n_rows = 0;
    std::vector<uint32_t> h_labels;            // the caller's labels of this shard's rows, until they are on the device
    const uint32_t* d_labels = nullptr;
    float *d_flag = nullptr, *d_dist = nullptr;
    unsigned long long *d_slots = nullptr, *d_words = nullptr;
    Event ev_slots;                            // shard >= 1: its slots hold global ids
};

// every shard's stream idle before the call's device memory goes, on every way out
struct Drain {
    std::vector<std::unique_ptr<SumShard>>& st;
    ~Drain() {
        for (auto& x : st)
            if (x && x->s) (void)hipStreamSynchronize(x->s);
    }
};

struct ShardedSummaryOut {
    std::vector<float> centroids, dist;
    std::vector<uint32_t> n;
    std::vector<uint64_t> slots;
    uint64_t outside = 0, unusable = 0;
};

// arguments checked, the table not empty; everything lands in `out`, dist by global row
void sharded_summary_run(ShardedCall& call, const uint32_t* labels, uint32_t C, bool want_centroids, bool want_dist,
                         ShardedSummaryOut* out) {
    mi_knn_sharded* t = call.t;
    const uint64_t G = t->rows;
    const uint32_t S = call.n, dim = t->dim;
    const size_t cbytes = (size_t)C * dim * sizeof(float), sbytes = (size_t)SUMMARY_PLANES * C * sizeof(unsigned long long);
    const uint32_t cblocks = (C + 255) / 256;
    std::vector<std::unique_ptr<SumShard>> st(S);
    for (uint32_t si = 0; si < S; ++si) st[si].reset(new SumShard);
    Drain drain{st};

    // labels to the shards, the rows that do not count, the shards' own sums.  (Not a TableCall: it would wait for the stream
    // where it closes; the stream is ordered behind the shard's earlier work by hand and settled with the results.)
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        std::lock_guard<std::mutex> l(sh->mu);
        DeviceGuard g(sh->device);
        SumShard& x = *st[si];
        x.sh = sh;
        x.n_rows = (uint32_t)sh->rows;
        x.map = knn_id_map(sh);
        x.s = knn_own_stream(sh);
        sh->writes.begin(x.s);
        sh->reads.begin(x.s);
        const uint32_t n = x.n_rows;
        x.ev.get(hipEventDisableTiming);
        x.ev_slots.get(hipEventDisableTiming);
        x.d_vec = (float*)x.scratch.get(cbytes);
        x.d_slots = (unsigned long long*)x.scratch.get(sbytes);
        HIP_CHECK(hipMemsetAsync(x.d_slots, 0xFF, (size_t)C * sizeof(unsigned long long), x.s));
        HIP_CHECK(hipMemsetAsync(x.d_slots + C, 0, (size_t)(SUMMARY_PLANES - 1) * C * sizeof(unsigned long long), x.s));
        if (si == 0) HIP_CHECK(hipMemsetAsync(x.d_vec, 0, cbytes, x.s));   // (the centroid kernel leaves an empty group's alone)
        if (n == 0) {   // it takes part in the exchange with zeros and untouched slots
            x.d_S = (long long*)x.scratch.get((size_t)C * dim * sizeof(long long));
            x.d_n = (uint32_t*)x.scratch.get((size_t)C * sizeof(uint32_t));
            HIP_CHECK(hipMemsetAsync(x.d_S, 0, (size_t)C * dim * sizeof(long long), x.s));
            HIP_CHECK(hipMemsetAsync(x.d_n, 0, (size_t)C * sizeof(uint32_t), x.s));
            if (si != 0) HIP_CHECK(hipEventRecord(x.ev, x.s));
            return;
        }
        if (labels) {
            x.h_labels.resize(n);
            summary_deal_labels(x.map, labels, n, x.h_labels.data());
            uint32_t* up = (uint32_t*)x.scratch.get((size_t)n * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(up, x.h_labels.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, x.s));
            x.d_labels = up;
        } else if (sh->d_groups) {
            x.d_labels = sh->d_groups;   // one id per row of capacity, MI_KNN_NO_GROUP where none was set
        } else {
            uint32_t* none = (uint32_t*)x.scratch.get((size_t)n * sizeof(uint32_t));
            HIP_CHECK(hipMemsetAsync(none, 0xFF, (size_t)n * sizeof(uint32_t), x.s));
            x.d_labels = none;
        }
        x.d_flag = (float*)x.scratch.get((size_t)n * sizeof(float));
        x.d_dist = (float*)x.scratch.get((size_t)n * sizeof(float));
        x.d_words = (unsigned long long*)x.scratch.get(SW_WORDS * sizeof(unsigned long long));
        x.u.alloc(x.scratch, n, C, dim, true);
        x.d_S = x.u.d_S;
        x.d_n = x.u.d_n;
        HIP_CHECK(hipMemsetAsync(x.d_words, 0, SW_WORDS * sizeof(unsigned long long), x.s));
        const uint64_t* tomb = sh->dead.empty() ? nullptr : sh->d_tomb;
        dispatch_nch(dim, [&](auto nch_c) {
            constexpr int NCH = decltype(nch_c)::value;
            hipLaunchKernelGGL((summary_prepare_kernel<NCH>), dim3(group16_blocks(sh, n)), dim3(256), 0, x.s, sh->table, x.d_labels, tomb, n,
                               C, x.u.d_inv, x.d_flag, x.d_dist, x.d_words);
            HIP_CHECK(hipGetLastError());
            x.u.template sums_fixed<NCH>(sh, x.s, x.d_labels, x.d_flag, n, C);
        });
        if (si != 0) HIP_CHECK(hipEventRecord(x.ev, x.s));
    });

    // the sums to shard 0 (it holds row 0: it is not empty), the centroids to every shard
    long long* d_in = nullptr;
    uint32_t* d_nin = nullptr;
    unsigned long long* d_sin = nullptr;
    if (S > 1) {
        DeviceGuard g(st[0]->sh->device);
        km_merge_staging(st[0]->scratch, C, dim, &d_in, &d_nin);
        d_sin = (unsigned long long*)st[0]->scratch.get(sbytes);
    }
    uint64_t merges = 0;
    std::vector<KmPart*> parts(S);
    for (uint32_t si = 0; si < S; ++si) parts[si] = st[si].get();
    km_merge_and_broadcast(parts, C, dim, d_in, d_nin, &merges);

    // the distances and the slots of every shard's members; the slots to global ids, then into shard 0's
    for (uint32_t si = 0; si < S; ++si) {
        SumShard& x = *st[si];
        std::lock_guard<std::mutex> l(x.sh->mu);
        DeviceGuard g(x.sh->device);
        if (x.n_rows != 0) {
            dispatch_nch(dim, [&](auto nch_c) {
                hipLaunchKernelGGL((summary_dist_kernel<decltype(nch_c)::value>), dim3(std::max(x.u.max_segs, 1u)), dim3(256), 0, x.s,
                                   x.sh->table, x.d_vec, x.u.d_sorted, x.u.d_start, x.u.d_seg, C, x.d_dist, x.d_slots);
            });
            hipLaunchKernelGGL(summary_globalize_kernel, dim3(cblocks), dim3(256), 0, x.s, x.d_slots, C, x.map);
            HIP_CHECK(hipGetLastError());
        }
        if (si != 0) HIP_CHECK(hipEventRecord(x.ev_slots, x.s));
    }
    {
        SumShard& z = *st[0];
        std::lock_guard<std::mutex> l(z.sh->mu);
        DeviceGuard g(z.sh->device);
        for (uint32_t si = 1; si < S; ++si) {
            SumShard& x = *st[si];
            HIP_CHECK(hipStreamWaitEvent(z.s, x.ev_slots, 0));
            copy_between(d_sin, z.sh->device, x.d_slots, x.sh->device, sbytes, z.s);
            hipLaunchKernelGGL(summary_merge_slots_kernel, dim3(cblocks), dim3(256), 0, z.s, z.d_slots, (const unsigned long long*)d_sin, C);
            HIP_CHECK(hipGetLastError());
            ++merges;
        }
    }

    // one wait per shard: dist to global rows; sizes, slots and centroids from shard 0; the counters and segments of all
    ShardedSummaryOut res;
    if (want_dist) res.dist.resize(G);
    if (want_centroids) res.centroids.resize((size_t)C * dim);
    res.n.resize(C);
    res.slots.resize((size_t)SUMMARY_PLANES * C);
    std::vector<uint32_t> segs(S, 0);
    std::vector<uint64_t> words((size_t)S * SW_WORDS, 0);
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        SumShard& x = *st[si];
        if (x.n_rows == 0) return;
        std::lock_guard<std::mutex> l(sh->mu);
        TableCall frame(sh);
        std::vector<float> dd(want_dist ? x.n_rows : 0);
        unsigned long long w[SW_WORDS] = {0, 0};
        if (want_dist) HIP_CHECK(hipMemcpyAsync(dd.data(), x.d_dist, (size_t)x.n_rows * sizeof(float), hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipMemcpyAsync(w, x.d_words, sizeof w, hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipMemcpyAsync(&segs[si], x.u.d_seg + C, sizeof(uint32_t), hipMemcpyDeviceToHost, x.s));
        if (si == 0) {
            HIP_CHECK(hipMemcpyAsync(res.n.data(), x.d_n, (size_t)C * sizeof(uint32_t), hipMemcpyDeviceToHost, x.s));
            HIP_CHECK(hipMemcpyAsync(res.slots.data(), x.d_slots, sbytes, hipMemcpyDeviceToHost, x.s));
            if (want_centroids) HIP_CHECK(hipMemcpyAsync(res.centroids.data(), x.d_vec, cbytes, hipMemcpyDeviceToHost, x.s));
        }
        HIP_CHECK(hipStreamSynchronize(x.s));
        if (want_dist) scatter_to_global(x.map, dd.data(), x.n_rows, res.dist.data());
        for (int i = 0; i < SW_WORDS; ++i) words[(size_t)si * SW_WORDS + i] = w[i];
    });
    for (uint32_t si = 0; si < S; ++si) {
        res.outside += words[(size_t)si * SW_WORDS + SW_OUTSIDE];
        res.unusable += words[(size_t)si * SW_WORDS + SW_UNUSABLE];
        t->summarize_stats[0] += segs[si];
    }
    t->summarize_stats[1] = summary_sharded_exchange_bytes(S, C, dim);
    t->summarize_stats[2] = merges;
    *out = std::move(res);
}

}  // namespace

extern "C" {

int mi_knn_sharded_summarize(mi_knn_sharded* t, const uint32_t* labels, uint32_t C, float* centroids, uint64_t* count, uint64_t* cover,
                             float* cover_dist, uint64_t* odd, float* odd_dist, uint64_t* measured, uint64_t* spread, float* dist,
                             uint64_t totals[4]) {
    return guarded([&] {
        // (mi_knn_summarize's rules, in front of anything that follows the handle)
        const char* why = "";
        const int bad = summary_check_args(t, C, &why);
        if (bad != MI_OK) fail(bad, "%s (got %u)", why, C);
        ShardedSummaryOut out;
        uint32_t block = 0;
        {
            ShardedCall call(t);
            check_mirror_dim(t->dim, "the summary's");
            if (!km_fixed_rows_ok(t->rows)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)t->rows);
            for (uint64_t& v : t->summarize_stats) v = 0;
            call.ready();
            if (t->rows == 0) {
                summary_pad(C, t->dim, centroids, count, cover, cover_dist, odd, odd_dist, measured, spread, totals);
                return;
            }
            block = t->block;
            sharded_summary_run(call, labels, C, centroids != nullptr, dist != nullptr, &out);
            for (uint32_t c = 0; c < C; ++c) t->summarize_stats[3] += out.n[c];
        }
        if (centroids) std::memcpy(centroids, out.centroids.data(), out.centroids.size() * sizeof(float));
        if (dist) std::memcpy(dist, out.dist.data(), out.dist.size() * sizeof(float));
        uint64_t members = 0, groups = 0;
        for (uint32_t c = 0; c < C; ++c) {
            members += out.n[c];
            groups += out.n[c] != 0;
            if (count) count[c] = out.n[c];
        }
        // the merged words carry global ids: the identity map (the sharded table has no base)
        summary_decode(out.slots.data(), out.n.data(), C, IdMap{0, block, 1, 0}, cover, cover_dist, odd, odd_dist, measured, spread);
        if (totals) {
            totals[0] = members; totals[1] = out.outside; totals[2] = out.unusable; totals[3] = groups;
        }
    });
}

int mi_knn_sharded_summarize_stats(mi_knn_sharded* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->summarize_stats[i];
    });
}

}  // extern "C"
