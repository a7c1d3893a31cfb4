// assign.hip — host side of mi_knn_assign (every row labelled by the nearest of C vectors), mi_knn_kmeans (Lloyd's
// iterations on top of it) and mi_knn_sharded_assign.  The call's state and argument rules: assign_call.h; the kernels and
// the superset argument: assign_kernels.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "assign_call.h"
#include "assign_kernels.h"
#include "kmeans_update.h"
#include "sharded_call.h"
#include "two_stage.h"

using namespace mi;

namespace {

// labels / dist of the shard's local rows
void assign_local(mi_knn* t, const float* vectors, uint32_t C, uint32_t* labels, float* dist) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->assign_stats) v = 0;
    if (t->rows == 0) return;
    Assign a;
    TableCall call(t);
    a.setup(call, C);
    HIP_CHECK(hipMemcpyAsync(a.d_vec, vectors, (size_t)C * t->dim * sizeof(float), hipMemcpyHostToDevice, a.s));
    a.run();
    HIP_CHECK(hipMemcpyAsync(labels, a.d_labels, (size_t)a.n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, a.s));
    if (dist) HIP_CHECK(hipMemcpyAsync(dist, a.d_dist, (size_t)a.n_rows * sizeof(float), hipMemcpyDeviceToHost, a.s));
    HIP_CHECK(hipStreamSynchronize(a.s));
}

template <int NCH>
void kmeans_loop(Assign& a, uint32_t max_iters, uint32_t* iters_run, uint64_t* changed_last) {
    KmUpdate u;   // d_labels / d_dist -> d_vec (kmeans_update.h)
    if (max_iters > 0) {
        u.alloc(a.scratch, a.n_rows, a.C, a.t->dim, a.t->kmeans_fixed_sum != 0);
        u.inv_norms<NCH>(a.t, a.s, a.n_rows);
    }
    uint32_t it = 0;
    uint64_t changed = 0;
    for (;;) {
        if (it == 0) {
            a.run();
            changed = (uint64_t)a.n_rows - a.t->dead.size();
        } else {
            a.run(true, &changed);
        }
        if ((it > 0 && changed == 0) || it == max_iters) break;
        u.run<NCH>(a.t, a.s, a.d_labels, a.d_dist, a.n_rows, a.C, a.d_vec);
        ++it;
    }
    *iters_run = it;
    *changed_last = changed;
}

}  // namespace

extern "C" {

int mi_knn_assign(mi_knn* t, const float* vectors, uint32_t C, uint32_t* labels, float* dist) {
    return guarded([&] {
        check_args(t, vectors, C, labels, true);
        assign_local(t, vectors, C, labels, dist);
    });
}

int mi_knn_assign_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->assign_stats[i];
    });
}

int mi_knn_kmeans(mi_knn* t, float* centroids, uint32_t C, uint32_t max_iters, uint32_t* labels, float* dist, uint32_t* iters_run,
                  uint64_t* changed_last, double* objective) {
    return guarded([&] {
        if (iters_run) *iters_run = 0;
        if (changed_last) *changed_last = 0;
        if (objective) *objective = 0.0;
        check_args(t, centroids, C, labels, false);
        std::lock_guard<std::mutex> l(t->mu);
        for (uint64_t& v : t->assign_stats) v = 0;
        if (t->rows == 0) return;
        Assign a;
        TableCall call(t);
        a.setup(call, C);
        const size_t cbytes = (size_t)C * t->dim * sizeof(float);
        HIP_CHECK(hipMemcpyAsync(a.d_vec, centroids, cbytes, hipMemcpyHostToDevice, a.s));
        uint32_t it = 0;
        uint64_t changed = 0;
        dispatch_nch(t->dim, [&](auto nch) { kmeans_loop<decltype(nch)::value>(a, max_iters, &it, &changed); });
        std::vector<uint32_t> h_labels;
        std::vector<float> h_dist;
        uint32_t* pl = labels;
        float* pd = dist;
        if (!pl) { h_labels.resize(a.n_rows); pl = h_labels.data(); }
        if (!pd) { h_dist.resize(a.n_rows); pd = h_dist.data(); }
        HIP_CHECK(hipMemcpyAsync(pl, a.d_labels, (size_t)a.n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, a.s));
        HIP_CHECK(hipMemcpyAsync(pd, a.d_dist, (size_t)a.n_rows * sizeof(float), hipMemcpyDeviceToHost, a.s));
        if (it > 0) HIP_CHECK(hipMemcpyAsync(centroids, a.d_vec, cbytes, hipMemcpyDeviceToHost, a.s));
        HIP_CHECK(hipStreamSynchronize(a.s));
        double obj = 0.0;   // in row order
        for (uint32_t r = 0; r < a.n_rows; ++r)
            if (pl[r] != MI_KNN_NO_LABEL && pd[r] == pd[r]) obj += (double)pd[r];
        if (iters_run) *iters_run = it;
        if (changed_last) *changed_last = changed;
        if (objective) *objective = obj;
    });
}

int mi_knn_sharded_assign(mi_knn_sharded* t, const float* vectors, uint32_t C, uint32_t* labels, float* dist) {
    return guarded([&] {
        ShardedCall call(t);
        check_args(t->shard[0], vectors, C, labels, true);
        // every shard on its own stream; results land at the rows' global ids
        call.for_each_shard([&](uint32_t, mi_knn* sh) {
            const uint64_t rows = sh->rows;
            std::vector<uint32_t> lab(rows);
            std::vector<float> dd(dist ? rows : 0);
            assign_local(sh, vectors, C, lab.data(), dist ? dd.data() : nullptr);
            const IdMap map = knn_id_map(sh);
            for (uint64_t r = 0; r < rows; ++r) {
                const uint64_t id = id_of_local(map, r);
                labels[id] = lab[r];
                if (dist) dist[id] = dd[r];
            }
        });
    });
}

}  // extern "C"
