// assign_call.h — one assign call's state (the rows' mirror built once, the vectors replaced per assign, the results on the
// device) and the argument rules of the calls built on it: mi_knn_assign, mi_knn_kmeans and mi_knn_sharded_assign (assign.hip),
// mi_knn_sharded_kmeans (kmeans_sharded.hip).  The kernels and the superset argument: assign_kernels.h.
#pragma once
#include <algorithm>

#include "assign_kernels.h"
#include "common.h"
#include "handles.h"
#include "two_stage.h"

namespace mi {

constexpr uint32_t ASSIGN_MAX_C = 65536;

// One call's state: the rows' mirror (built once), the vectors (replaced per assign), the results on the device.
struct Assign {
    mi_knn* t = nullptr;
    hipStream_t s = nullptr;
    Scratch scratch;
    uint32_t n_rows = 0, C = 0, n_cb = 0, cand_cap = 0;
    float thr = 0.0f;
    const uint16_t* mirror = nullptr;
    const float* xx = nullptr;
    const uint64_t* tomb = nullptr;
    float* d_vec = nullptr;          // [C][dim] fp32
    uint16_t* d_vmirror = nullptr;
    float* d_vxx = nullptr;
    uint2* d_cand = nullptr;
    unsigned long long *d_count = nullptr, *d_best = nullptr, *d_changed = nullptr;
    uint32_t* d_labels = nullptr;
    float* d_dist = nullptr;
    uint32_t strip = 0;
    uint64_t stats[4] = {0, 0, 0, 0};

    template <int NCH>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) {
            static DevOnce once;
            allow_lds_once(once, assign_tiles_kernel<NCH>, ASG_LDS);
            HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL((assign_tiles_kernel<NCH>), dim3(r1 - r0), dim3(256), ASG_LDS, s, mirror, xx, tomb, n_rows, d_vmirror,
                               d_vxx, C, r0, c0, c1, thr, cand_cap, d_cand, d_count);
            HIP_CHECK(hipGetLastError());
            ++stats[2];
            stats[3] += (uint64_t)(r1 - r0) * (c1 - c0);
            return read_count(d_count, s);
        };
        auto stage2 = [&](uint32_t n) {   // (the rows' minima live in d_best: they join the pieces of a row)
            stats[0] += n;
            hipLaunchKernelGGL((assign_rescore_kernel<NCH>), dim3(group16_blocks(t, n)), dim3(256), 0, s, t->table, d_vec, d_cand, n,
                               d_best);
            HIP_CHECK(hipGetLastError());
        };
        rect_stages(br0, br1, bc0, bc1, cand_cap, overflowed, stage1, stage2);
    }

    // d_vec holds the vectors: -> d_labels / d_dist.  prev_in_labels: count the rows whose label changes into *changed
    template <int NCH>
    void run(bool count_changed, uint64_t* changed) {
        for (uint64_t& v : stats) v = 0;
        mirror_rows(t, s, d_vec, 0, C, d_vmirror, d_vxx);
        HIP_CHECK(hipMemsetAsync(d_best, 0xFF, (size_t)n_rows * sizeof(unsigned long long), s));
        const uint32_t n_rb = (n_rows + TILE - 1) / TILE;
        // strips of row tiles: as many as keep an ordinary corpus (a few candidates per row and column tile) inside the buffer
        if (strip == 0) strip = std::max<uint32_t>(1u, std::min<uint32_t>(2048u, cand_cap / (TILE * 4u * n_cb)));
        for (uint32_t br = 0; br < n_rb;) {
            const uint32_t end = std::min(n_rb, br + strip);
            bool overflowed = false;
            rect<NCH>(br, end, 0, n_cb, &overflowed);
            if (overflowed) strip = std::max(1u, strip / 2);
            br = end;
        }
        if (count_changed) HIP_CHECK(hipMemsetAsync(d_changed, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(assign_finalize_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, d_best, tomb, n_rows,
                           count_changed ? d_labels : (const uint32_t*)nullptr, d_labels, d_dist, d_changed);
        HIP_CHECK(hipGetLastError());
        if (count_changed) {
            unsigned long long c = 0;
            HIP_CHECK(hipMemcpyAsync(&c, d_changed, sizeof c, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            *changed = c;
        }
        stats[1] = (uint64_t)n_rows - t->dead.size();
        for (int i = 0; i < 4; ++i) t->assign_stats[i] = stats[i];
    }

    void run(bool count_changed = false, uint64_t* changed = nullptr) {
        dispatch_nch(t->dim, [&](auto nch) { run<decltype(nch)::value>(count_changed, changed); });
    }

    // inside the call's frame (declared after this object: the stream is idle before the scratch memory goes); arguments
    // checked, the table not empty
    void setup(const TableCall& call, uint32_t n_vec) {
        t = call.t;
        C = n_vec;
        s = call.s;
        n_rows = (uint32_t)t->rows;
        n_cb = (C + TILE - 1) / TILE;
        thr = 2.0f * eps2(t->dim);   // the join's bound, unchanged (join_kernels.h): both operands are rounded to bf16
        cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
        const TableMirror tm = table_mirror(t, s, scratch);
        mirror = tm.mirror; xx = tm.xx; tomb = tm.tomb;
        d_vec = (float*)scratch.get((size_t)C * t->dim * sizeof(float));
        d_vmirror = (uint16_t*)scratch.get((size_t)C * t->dim * sizeof(uint16_t));
        d_vxx = (float*)scratch.get((size_t)C * sizeof(float));
        d_cand = (uint2*)scratch.get((size_t)cand_cap * sizeof(uint2));
        d_count = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
        d_changed = d_count + 1;
        d_best = (unsigned long long*)scratch.get((size_t)n_rows * sizeof(unsigned long long));
        d_labels = (uint32_t*)scratch.get((size_t)n_rows * sizeof(uint32_t));
        d_dist = (float*)scratch.get((size_t)n_rows * sizeof(float));
    }
};

inline void check_args(const mi_knn* t, const float* vectors, uint32_t C, const uint32_t* labels, bool labels_needed) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (!vectors) fail(MI_ERR_INVALID, "vectors is null");
    if (labels_needed && !labels) fail(MI_ERR_INVALID, "labels is null");
    if (C == 0) fail(MI_ERR_INVALID, "C must be >= 1");
    if (C > ASSIGN_MAX_C) fail(MI_ERR_UNSUPPORTED, "at most %u vectors (got %u)", ASSIGN_MAX_C, C);
    check_mirror_dim(t->dim, "the assign's");
}

}  // namespace mi
