// ordered.hip — host side of mi_knn_search_ordered and mi_knn_stamp_histogram: the rows within a distance in the order of their
// stamps — "everything that looks like this, newest first, 100 at a time" — and the timeline facet over the same rows.  The
// kernels, and why the selection key is (okey(stamp), position): ordered_kernels.h.  The host-only rules: ordered_host.h.
//
// One call: with a predicate its passes leave the ascending list of the rows it keeps (knn_filter_where); the query goes up;
// the paged search's scan in its one-key-per-entry form (knn_page_scan_keys32) classifies every candidate against the bound;
// nine short histogram passes (most of which return at once), a collect, a one-block sort and ordered_finish_kernel turn the
// keys into ids, distances and stamps beside the counts, and the host copies that one record back in one piece.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "ordered_host.h"
#include "ordered_kernels.h"
#include "page_host.h"
#include "scan_call.h"
#include "two_stage.h"

using namespace mi;

namespace {

// What both calls share in front of their own passes: the candidates (w: the predicate's list, built here on the device, else the
// table under its deletion bitmap), the query, the scan.  Leaves one distance key per entry in keys32 (the caller's scan_keys32
// of the table's rows) and {-, within, beyond, nan} added to d_counts (zeroed here); n == 0: no candidate, nothing was launched
// behind the predicate.  t->mu held, inside the call's frame
ScanSet scan_candidates(mi_knn* t, const float* q, float max_dist, const mi_knn_where* w, uint32_t k, hipStream_t s, uint32_t* keys32,
                        unsigned long long* d_counts) {
    if (w) knn_filter_where(t, w, s);
    const ScanSet c = scan_set(t, s, w ? SCAN_DEVICE_LIST : SCAN_TABLE);
    if (c.n == 0) return c;
    HIP_CHECK(hipMemcpyAsync(t->d_q, q, (size_t)t->dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_counts, 0, 4 * sizeof(uint64_t), s));
    knn_page_scan_keys32(t, s, c.n, c.list, c.tomb, page_hi(max_dist), k, keys32, d_counts);
    return c;
}

}  // namespace

namespace mi {

// the call behind the C entry points (arguments checked by ordered_check_args); throws Error.  cur (nullable): the cursor as a
// shard takes it from the sharded call; otherwise it is built here from (flags, after_stamp, after_id), and after_id must name a
// row of t
void knn_search_ordered(mi_knn* t, const float* q, uint32_t k, float max_dist, const mi_knn_where* w, uint32_t flags, int64_t after_stamp,
                        uint64_t after_id, const OrderedCursor* cur_in, uint64_t* idx, float* dist, int64_t* stamps, uint64_t* counts) {
    std::lock_guard<std::mutex> l(t->mu);
    check_scan_dim(t->dim, "the ordered search");
    OrderedCursor cur;
    if (cur_in) cur = *cur_in;
    else if (!ordered_cursor(knn_id_map(t), t->rows, flags, after_stamp, after_id, &cur))
        fail(MI_ERR_INVALID, "after_id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)after_id,
             (unsigned long long)t->base, (unsigned long long)t->rows);
    if (t->rows == 0 || (w && where_never(*w, t->d_groups != nullptr))) {
        ordered_pad(k, idx, dist, stamps, counts);
        return;
    }

    TableCall call(t);
    hipStream_t s = call.s;
    const OrderedRecord rec = ordered_record(k);
    unsigned char* d_rec = scan_record(t, rec.bytes);
    t->d_keys.reserve(t->reads, (size_t)ORDERED_K_MAX * 2);   // sorted: hi [4096] | lo [4096]
    t->d_cand.reserve(t->reads, (size_t)ORDERED_K_MAX * 2);  // collected: the same
    t->d_sel.reserve(t->reads, ORD_SEL_WORDS);
    uint32_t* keys32 = scan_keys32(t, t->rows);

    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(d_rec + rec.counts);
    const ScanSet c = scan_candidates(t, q, max_dist, w, k, s, keys32, d_counts);
    const uint64_t n = c.n;
    const uint32_t* list = c.list;
    if (n == 0) {
        ordered_pad(k, idx, dist, stamps, counts);
        return;
    }
    HIP_CHECK(hipMemsetAsync(t->d_sel, 0, ORD_SEL_WORDS * sizeof(uint32_t), s));
    uint32_t* d_hist = t->d_sel;
    OrdState* d_states = reinterpret_cast<OrdState*>(t->d_sel + ORD_HIST_WORDS);
    uint32_t* d_count = t->d_sel + ORD_HIST_WORDS + ORD_STATE_WORDS;
    uint64_t* c_hi = t->d_cand;
    uint32_t* c_lo = reinterpret_cast<uint32_t*>(t->d_cand + ORDERED_K_MAX);
    uint64_t* s_hi = t->d_keys;
    uint32_t* s_lo = reinterpret_cast<uint32_t*>(t->d_keys + ORDERED_K_MAX);
    const long long* d_stamps = reinterpret_cast<const long long*>(t->d_stamps.p);
    // one entry per thread and round; the grid rule (and the option) of the scan in front
    const uint32_t blocks = scan_grid(n, t->n_cu, t->page_blocks, PAGE_BLOCKS_PER_CU);
    for (int p = 0; p < ORD_PASSES; ++p) {
        hipLaunchKernelGGL(ordered_hist_kernel, dim3(blocks), dim3(256), 0, s, keys32, n, list, d_stamps, cur, k, p, d_hist, d_states,
                           d_counts);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ordered_collect_kernel, dim3(blocks), dim3(256), 0, s, keys32, n, list, d_stamps, cur, k, d_hist, d_states, c_hi,
                       c_lo, d_count);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ordered_sort_kernel, dim3(1), dim3(1024), 0, s, c_hi, c_lo, d_count, k, s_hi, s_lo);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ordered_finish_kernel, dim3((k + 255) / 256), dim3(256), 0, s, s_hi, s_lo, d_count, k, keys32, list, (int)cur.desc,
                       knn_id_map(t), reinterpret_cast<uint64_t*>(d_rec + rec.idx), reinterpret_cast<float*>(d_rec + rec.dist),
                       reinterpret_cast<long long*>(d_rec + rec.stamps));
    HIP_CHECK(hipGetLastError());
    ordered_unpack(scan_record_fetch(d_rec, rec.bytes, s).data(), k, idx, dist, stamps, counts);
}

// mi_knn_stamp_histogram behind its argument check; hist [n_edges + 1] is written only on success
void knn_stamp_histogram(mi_knn* t, const float* q, float max_dist, const mi_knn_where* w, const int64_t* edges, uint32_t n_edges,
                         uint64_t* hist) {
    std::lock_guard<std::mutex> l(t->mu);
    check_scan_dim(t->dim, "the stamp histogram");
    const size_t bins = (size_t)n_edges + 1;
    if (t->rows == 0 || (w && where_never(*w, t->d_groups != nullptr))) {
        std::fill(hist, hist + bins, 0ull);
        return;
    }
    TableCall call(t);
    hipStream_t s = call.s;
    unsigned char* d_rec = scan_record(t, (bins + 4) * sizeof(uint64_t));                             // hist [bins] | the scan's counts [4]
    t->d_keys.reserve(t->reads, (size_t)ORDERED_K_MAX * 2);   // the edges
    uint32_t* keys32 = scan_keys32(t, t->rows);

    unsigned long long* d_hist = reinterpret_cast<unsigned long long*>(d_rec);
    const ScanSet c = scan_candidates(t, q, max_dist, w, 1, s, keys32, d_hist + bins);
    if (c.n == 0) {
        std::fill(hist, hist + bins, 0ull);
        return;
    }
    HIP_CHECK(hipMemsetAsync(d_hist, 0, bins * sizeof(uint64_t), s));
    HIP_CHECK(hipMemcpyAsync(t->d_keys, edges, (size_t)n_edges * sizeof(int64_t), hipMemcpyHostToDevice, s));
    const uint32_t blocks = scan_grid(c.n, t->n_cu, t->page_blocks, PAGE_BLOCKS_PER_CU);
    hipLaunchKernelGGL(ordered_stamp_hist_kernel, dim3(blocks), dim3(256), 0, s, keys32, c.n, c.list,
                       reinterpret_cast<const long long*>(t->d_stamps.p), reinterpret_cast<const long long*>(t->d_keys.p), n_edges, d_hist);
    HIP_CHECK(hipGetLastError());
    // hist is written only on success: the bins come to the host first
    std::memcpy(hist, scan_record_fetch(d_rec, bins * sizeof(uint64_t), s).data(), bins * sizeof(uint64_t));
}

}  // namespace mi

extern "C" {

int mi_knn_search_ordered(mi_knn* t, const float* q, uint32_t k, float max_dist, const mi_knn_where* w, uint32_t flags, int64_t after_stamp,
                          uint64_t after_id, uint64_t* idx, float* dist, int64_t* stamps, uint64_t counts[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = ordered_check_args(t, q, k, max_dist, w, flags, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        knn_search_ordered(t, q, k, max_dist, w, flags, after_stamp, after_id, nullptr, idx, dist, stamps, counts);
    });
}

int mi_knn_stamp_histogram(mi_knn* t, const float* q, float max_dist, const mi_knn_where* w, const int64_t* edges, uint32_t n_edges,
                           uint64_t* hist) {
    return guarded([&] {
        const char* why = "";
        const int bad = ordered_check_hist_args(t, q, max_dist, w, edges, n_edges, hist, &why);
        if (bad != MI_OK) fail(bad, "%s (n_edges %u)", why, n_edges);
        knn_stamp_histogram(t, q, max_dist, w, edges, n_edges, hist);
    });
}

}  // extern "C"
