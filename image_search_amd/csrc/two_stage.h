// two_stage.h — host side shared by the calls whose first stage is the 128 x 128 bf16 tile (tile128.h) and whose second
// stage rescoring decides in the search's arithmetic: the join, the assign, the multi-label assign and the many-query
// search.  The table's mirror for the call, the dispatch over the dims the mirror is built for,
// and the scheme that redoes a launch whose candidates overflowed the buffer.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "handles.h"
#include "knn_shared.h"
#include "scan_call.h"   // Settle, the frame of a call (TableCall), the dim rule

namespace mi {

// n elements of a call's device array into a host vector, enqueued on s (the caller waits for the stream)
template <class T>
void read_back(std::vector<T>* v, const T* d, size_t n, hipStream_t s) {
    v->resize(n);
    HIP_CHECK(hipMemcpyAsync(v->data(), d, n * sizeof(T), hipMemcpyDeviceToHost, s));
}
// a call's result into the caller's array, which may be null, once the call's frame has left
template <class T>
void copy_out(const std::vector<T>& v, T* p) {
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
}

// The bound of a first stage with BOTH operands rounded to bf16 (derived in join_kernels.h):
// |coarse - exact| <= eps2 on the cosine of every pair the mirror does not mark.
inline float eps2(uint32_t dim) { return 0x1p-7f + 0x1p-16f + 4.1f * (float)(dim + 8) * 0x1p-24f + 2e-6f; }

// `whose`: "the join's", "the assign's", ... for the message
inline void check_mirror_dim(uint32_t dim, const char* whose) { check_scan_dim(dim, (std::string(whose) + " bf16 mirror").c_str()); }

// f(std::integral_constant<int, NCH>) with NCH = dim / 64; dim has passed check_mirror_dim
template <class F>
void dispatch_nch(uint32_t dim, F&& f) {
    switch (dim / 64) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 12: f(std::integral_constant<int, 12>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
    }
}

// workgroups of a kernel that gives each of n items a 16-lane group and strides over them
inline uint32_t group16_blocks(const mi_knn* t, uint64_t n) {
    return std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 8, (n + 15) / 16));
}

// rows [from, end) of `rows` -> bf16 mirror rows + stored squared norms
inline void mirror_rows(mi_knn* t, hipStream_t s, const float* rows, uint64_t from, uint64_t end, uint16_t* mirror, float* xx) {
    dispatch_nch(t->dim, [&](auto nch) {
        hipLaunchKernelGGL((knn_mirror_kernel<decltype(nch)::value>), dim3(group16_blocks(t, end - from)), dim3(256), 0, s, rows, from, end,
                           mirror, xx);
    });
    HIP_CHECK(hipGetLastError());
}

// The table's mirror for this call: the table's own when "prefilter" = 1 keeps one (caught up here as a search would), else
// one built for the call in `scratch`.  tomb: the deleted rows' bits, null when there are none.  t->mu held, t not empty.
struct TableMirror {
    const uint16_t* mirror;
    const float* xx;
    const uint64_t* tomb;
};
inline TableMirror table_mirror(mi_knn* t, hipStream_t s, Scratch& scratch) {
    uint16_t* m = nullptr;
    float* x = nullptr;
    uint64_t from = 0;
    if (t->prefilter == 1) {
        t->mirror_rows = std::min(t->mirror_rows, t->rows);
        // the table's own mirror grows with its capacity, keeping the rows mirrored so far (what the two-stage search does)
        t->d_mirror.reserve_keep(t->reads, (size_t)t->cap * t->dim, (size_t)t->mirror_rows * t->dim);
        t->d_xx.reserve_keep(t->reads, (size_t)t->cap, (size_t)t->mirror_rows);
        m = t->d_mirror; x = t->d_xx; from = t->mirror_rows;
    } else {
        m = (uint16_t*)scratch.get((size_t)t->rows * t->dim * sizeof(uint16_t));
        x = (float*)scratch.get((size_t)t->rows * sizeof(float));
    }
    if (from < t->rows) {
        mirror_rows(t, s, t->table, from, t->rows, m, x);
        if (t->prefilter == 1) t->mirror_rows = t->rows;
    }
    return TableMirror{m, x, t->dead.empty() ? nullptr : t->d_tomb};
}

// Stage 1 and stage 2 over the tiles [br0, br1) x [bc0, bc1) with a candidate buffer of `cap`.
//   stage1(br0, br1, bc0, bc1) launches stage 1 on the rectangle and returns the candidates it COUNTED (the buffer holds
//       the first cap of them).  bc0 is passed by reference: the join raises it to the diagonal.
//   stage2(n) consumes the buffer's n <= cap candidates.
// More than cap: nothing is dropped and nothing consumed — the same ground again in two halves, rows first, then columns
// (whatever stage 2 keeps per row must therefore join the pieces of a row).  *overflowed (nullable) is set then.
template <class Stage1, class Stage2>
void rect_stages(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, uint32_t cap, bool* overflowed, Stage1& stage1, Stage2& stage2) {
    if (bc0 >= bc1 || br0 >= br1) return;
    const unsigned long long n_cand = stage1(br0, br1, bc0, bc1);
    if (n_cand > cap) {
        if (overflowed) *overflowed = true;
        if (br1 - br0 > 1) {
            const uint32_t mid = br0 + (br1 - br0) / 2;
            rect_stages(br0, mid, bc0, bc1, cap, nullptr, stage1, stage2);
            rect_stages(mid, br1, bc0, bc1, cap, nullptr, stage1, stage2);
        } else if (bc1 - bc0 > 1) {
            const uint32_t mid = bc0 + (bc1 - bc0) / 2;
            rect_stages(br0, br1, bc0, mid, cap, nullptr, stage1, stage2);
            rect_stages(br0, br1, mid, bc1, cap, nullptr, stage1, stage2);
        } else {
            fail(MI_ERR_INVALID, "one tile reported %llu candidates (the buffer holds %u)", n_cand, cap);
        }
        return;
    }
    if (n_cand) stage2((uint32_t)n_cand);
}

// the candidates a stage-1 launch counted into *d_count, read back (the stream is idle afterwards)
inline unsigned long long read_count(const unsigned long long* d_count, hipStream_t s) {
    unsigned long long n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, d_count, sizeof n, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return n;
}

}  // namespace mi
