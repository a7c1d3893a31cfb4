// kmeans_sharded.hip — host side of mi_knn_sharded_kmeans and mi_knn_sharded_kmeans_stats: Lloyd's iterations of mi_knn_kmeans
// over a block-cyclic table.  Every shard assigns its own rows (assign_call.h) and sums them per cluster as exact integers of
// 2^-30 (kmeans_update.h, assign_kernels.h); the sums and sizes of shards 1 .. S - 1 are copied to shard 0's device and added
// into shard 0's, the centroids are formed there and go back to every shard.  Integer sums are the same in any order, so the
// result is the single table's with "kmeans_fixed_sum" = 1, bit for bit, whatever the layout.  The rules without HIP in them:
// kmeans_fixed_host.h.
//
// Streams: a shard's work runs on its own stream.  In an update, shard 0's stream waits for the event behind every other
// shard's sums, and every other shard's stream waits for the event behind the centroids before it copies them; the host
// waits only where mi_knn_kmeans does, for an assign's candidate and changed counts.
#include <algorithm>
#include <cstring>

#include <memory>
#include <mutex>
#include <vector>

#include "assign_call.h"
#include "common.h"
#include "density_sharded_host.h"   // scatter_to_global
#include "handles.h"
#include "kmeans_fixed_host.h"
#include "kmeans_sharded_merge.h"
#include "kmeans_update.h"
#include "sharded_call.h"
#include "two_stage.h"

using namespace mi;

namespace {

// one shard's state for the call; its device memory lives in a.scratch, on the shard's device.  d_vec is a.d_vec and d_S /
// d_n are u's where the shard has rows
struct KmShard : KmPart {
    Assign a;
    KmUpdate u;
    IdMap map{0, 0, 0, 0};
    uint32_t n_rows = 0;
};

// every shard's stream idle before the call's device memory goes, on every way out
struct Drain {
    std::vector<std::unique_ptr<KmShard>>& st;
    ~Drain() {
        for (auto& x : st)
            if (x && x->s) (void)hipStreamSynchronize(x->s);
    }
};

struct ShardedKmeansOut {
    std::vector<uint32_t> labels;
    std::vector<float> dist, centroids;
    uint32_t iters = 0;
    uint64_t changed = 0;
    double objective = 0.0;
};

// One update: st[si]'s labels / dist -> the centroids in every shard's d_vec.  Enqueues only; t->mu held.
void update_round(mi_knn_sharded* t, std::vector<std::unique_ptr<KmShard>>& st, uint32_t C, long long* d_in, uint32_t* d_nin,
                  uint64_t* merges) {
    const uint32_t S = t->n(), dim = t->dim;
    for (uint32_t si = 0; si < S; ++si) {
        KmShard& x = *st[si];
        std::lock_guard<std::mutex> l(x.sh->mu);
        DeviceGuard g(x.sh->device);
        if (x.n_rows != 0)
            dispatch_nch(dim, [&](auto nch) { x.u.template sums_fixed<decltype(nch)::value>(x.sh, x.s, x.a.d_labels, x.a.d_dist, x.n_rows, C); });
        if (si != 0) HIP_CHECK(hipEventRecord(x.ev, x.s));
    }
    std::vector<KmPart*> parts(S);
    for (uint32_t si = 0; si < S; ++si) parts[si] = st[si].get();
    km_merge_and_broadcast(parts, C, dim, d_in, d_nin, merges);   // kmeans_sharded_merge.h
}

// arguments checked; everything lands in `out`, by global row
void sharded_kmeans_run(ShardedCall& call, const float* centroids, uint32_t C, uint32_t max_iters, ShardedKmeansOut* out) {
    mi_knn_sharded* t = call.t;
    for (uint64_t& v : t->kmeans_stats) v = 0;
    check_mirror_dim(t->dim, "the assign's");
    if (!km_fixed_rows_ok(t->rows)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)t->rows);
    call.ready();
    const uint64_t G = t->rows;
    if (G == 0) return;
    const uint32_t S = call.n, dim = t->dim;
    const size_t cbytes = (size_t)C * dim * sizeof(float);
    std::vector<std::unique_ptr<KmShard>> st(S);
    for (uint32_t si = 0; si < S; ++si) st[si].reset(new KmShard);
    Drain drain{st};

    // the shards' state: the rows' mirror and 1 / |x| once, the start centroids
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        std::lock_guard<std::mutex> l(sh->mu);
        KmShard& x = *st[si];
        x.sh = sh;
        x.n_rows = (uint32_t)sh->rows;
        x.map = knn_id_map(sh);
        for (uint64_t& v : sh->assign_stats) v = 0;
        if (x.n_rows == 0) {   // it takes part in the exchange with zeros
            DeviceGuard g(sh->device);
            x.s = knn_own_stream(sh);
            x.ev.get(hipEventDisableTiming);
            x.d_vec = (float*)x.a.scratch.get(cbytes);
            x.d_S = (long long*)x.a.scratch.get((size_t)C * dim * sizeof(long long));
            x.d_n = (uint32_t*)x.a.scratch.get((size_t)C * sizeof(uint32_t));
            HIP_CHECK(hipMemsetAsync(x.d_S, 0, (size_t)C * dim * sizeof(long long), x.s));
            HIP_CHECK(hipMemsetAsync(x.d_n, 0, (size_t)C * sizeof(uint32_t), x.s));
            HIP_CHECK(hipStreamSynchronize(x.s));
            return;
        }
        TableCall call(sh);
        x.s = call.s;
        x.ev.get(hipEventDisableTiming);
        x.a.setup(call, C);
        x.d_vec = x.a.d_vec;
        HIP_CHECK(hipMemcpyAsync(x.d_vec, centroids, cbytes, hipMemcpyHostToDevice, x.s));
        if (max_iters > 0) {
            x.u.alloc(x.a.scratch, x.n_rows, C, dim, true);
            x.d_S = x.u.d_S;
            x.d_n = x.u.d_n;
            dispatch_nch(dim, [&](auto nch) { x.u.template inv_norms<decltype(nch)::value>(sh, x.s, x.n_rows); });
        }
    });

    // shard 0 (it holds row 0: it is not empty) stages the other shards' sums
    long long* d_in = nullptr;
    uint32_t* d_nin = nullptr;
    if (max_iters > 0 && S > 1) {
        DeviceGuard g(st[0]->sh->device);
        km_merge_staging(st[0]->a.scratch, C, dim, &d_in, &d_nin);
    }

    uint64_t dead = 0;
    for (uint32_t si = 0; si < S; ++si) dead += t->shard[si]->dead.size();
    uint32_t it = 0;
    uint64_t changed = 0, merges = 0;
    std::vector<uint64_t> ch(S);
    for (;;) {
        std::fill(ch.begin(), ch.end(), 0);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            KmShard& x = *st[si];
            if (x.n_rows == 0) return;
            std::lock_guard<std::mutex> l(sh->mu);
            TableCall call(sh);
            if (it == 0) x.a.run();
            else x.a.run(true, &ch[si]);
        });
        if (it == 0) {
            changed = G - dead;
        } else {
            changed = 0;
            for (uint64_t c : ch) changed += c;
        }
        if ((it > 0 && changed == 0) || it == max_iters) break;   // mi_knn_kmeans' stop rule
        update_round(t, st, C, d_in, d_nin, &merges);
        ++it;
    }

    // labels and dist to global rows; the centroids from shard 0; the segments of the last update
    ShardedKmeansOut res;
    res.labels.assign(G, MI_KNN_NO_LABEL);
    res.dist.assign(G, 0.0f);
    if (it > 0) res.centroids.resize((size_t)C * dim);
    std::vector<uint32_t> segs(S, 0);
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        KmShard& x = *st[si];
        if (x.n_rows == 0) return;
        std::lock_guard<std::mutex> l(sh->mu);
        TableCall call(sh);
        std::vector<uint32_t> lab(x.n_rows);
        std::vector<float> dd(x.n_rows);
        HIP_CHECK(hipMemcpyAsync(lab.data(), x.a.d_labels, (size_t)x.n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipMemcpyAsync(dd.data(), x.a.d_dist, (size_t)x.n_rows * sizeof(float), hipMemcpyDeviceToHost, x.s));
        if (it > 0) HIP_CHECK(hipMemcpyAsync(&segs[si], x.u.d_seg + C, sizeof(uint32_t), hipMemcpyDeviceToHost, x.s));
        if (it > 0 && si == 0) HIP_CHECK(hipMemcpyAsync(res.centroids.data(), x.d_vec, cbytes, hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipStreamSynchronize(x.s));
        scatter_to_global(x.map, lab.data(), x.n_rows, res.labels.data());
        scatter_to_global(x.map, dd.data(), x.n_rows, res.dist.data());
    });
    double obj = 0.0;   // in global row order
    for (uint64_t r = 0; r < G; ++r)
        if (res.labels[r] != MI_KNN_NO_LABEL && res.dist[r] == res.dist[r]) obj += (double)res.dist[r];
    res.iters = it;
    res.changed = changed;
    res.objective = obj;
    t->kmeans_stats[0] = it;
    t->kmeans_stats[1] = (uint64_t)it * km_fixed_exchange_bytes(S, C, dim);
    for (uint32_t si = 0; si < S; ++si) t->kmeans_stats[2] += segs[si];
    t->kmeans_stats[3] = merges;
    *out = std::move(res);
}

}  // namespace

extern "C" {

int mi_knn_sharded_kmeans(mi_knn_sharded* t, float* centroids, uint32_t C, uint32_t max_iters, uint32_t* labels, float* dist,
                          uint32_t* iters_run, uint64_t* changed_last, double* objective) {
    return guarded([&] {
        // (mi_knn_kmeans' rules, in front of anything that follows the handle)
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (!centroids) fail(MI_ERR_INVALID, "vectors is null");
        if (C == 0) fail(MI_ERR_INVALID, "C must be >= 1");
        if (C > ASSIGN_MAX_C) fail(MI_ERR_UNSUPPORTED, "at most %u vectors (got %u)", ASSIGN_MAX_C, C);
        ShardedKmeansOut out;
        {
            ShardedCall call(t);
            sharded_kmeans_run(call, centroids, C, max_iters, &out);
        }
        if (labels && !out.labels.empty()) std::memcpy(labels, out.labels.data(), out.labels.size() * sizeof(uint32_t));
        if (dist && !out.dist.empty()) std::memcpy(dist, out.dist.data(), out.dist.size() * sizeof(float));
        if (!out.centroids.empty()) std::memcpy(centroids, out.centroids.data(), out.centroids.size() * sizeof(float));
        if (iters_run) *iters_run = out.iters;
        if (changed_last) *changed_last = out.changed;
        if (objective) *objective = out.objective;
    });
}

int mi_knn_sharded_kmeans_stats(mi_knn_sharded* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->kmeans_stats[i];
    });
}

}  // extern "C"
