// page.hip — host side of mi_knn_search_page: the k nearest rows AFTER a cursor and WITHIN a distance, with the counts of the
// candidates before, inside and beyond that window, exact, in one pass over the fp32 rows.
// The kernels, and why the window is applied on keys: page_kernels.h.  The host-only rules: page_host.h.
//
// One call: the query goes up; knn_page_scan_kernel classifies every candidate and leaves per-wave lists (k <= 64, reduced by
// the search's merge tree) or one distance key per row (k > 64, the search's radix select); knn_page_finish_kernel turns the
// k keys into ids and distances beside the counts, and the host copies that one record back in one piece.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "compound_host.h"
#include "handles.h"
#include "page_host.h"
#include "page_kernels.h"
#include "two_stage.h"

using namespace mi;

namespace {

template <int NCH>
void launch_scan(mi_knn* t, uint32_t blocks, hipStream_t s, uint64_t n, const uint32_t* list, const uint64_t* tomb, uint64_t first_key,
                 uint64_t hi, uint32_t k, uint64_t* cand, uint32_t* all_keys, unsigned long long* counts) {
    if (all_keys)
        hipLaunchKernelGGL((knn_page_scan_kernel<NCH, 1>), dim3(blocks), dim3(256), 0, s, t->table, n, list, tomb, t->d_q, first_key, hi, k,
                           cand, all_keys, counts);
    else
        hipLaunchKernelGGL((knn_page_scan_kernel<NCH, 0>), dim3(blocks), dim3(256), 0, s, t->table, n, list, tomb, t->d_q, first_key, hi, k,
                           cand, all_keys, counts);
    HIP_CHECK(hipGetLastError());
}

PageIds page_ids(const mi_knn* t) { return PageIds{t->base, t->rows, t->cyc_block, t->cyc_n, t->cyc_rank}; }

}  // namespace

namespace mi {

// the scan without a cursor in its one-key-per-row form, for the grouped search (grouped.hip): keys32 [n] = the distance key of
// every row or list entry, 0xFFFFFFFF outside the window [0, hi]; counts += {0, window, beyond, nan}.  t->mu held, device
// selected, the query in t->d_q
void knn_page_scan_keys32(mi_knn* t, hipStream_t s, uint64_t n, const uint32_t* list, const uint64_t* tomb, uint64_t hi, uint32_t k,
                          uint32_t* keys32, unsigned long long* counts) {
    const uint32_t blocks = page_grid(n, t->n_cu, t->page_blocks);
    dispatch_nch(t->dim, [&](auto nch) { launch_scan<decltype(nch)::value>(t, blocks, s, n, list, tomb, 0, hi, k, nullptr, keys32, counts); });
}

// the call behind the C entry points (arguments checked by page_check_args); throws Error.  cursor_is_id: first_key is built
// here from (after_dist, after_id), which must name a row of t; otherwise the caller — the sharded call — hands first_key over.
void knn_search_page(mi_knn* t, const float* q, uint32_t k, bool cursor_is_id, float after_dist, uint64_t after_id, uint64_t first_key,
                     float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, uint64_t* counts) {
    std::lock_guard<std::mutex> l(t->mu);
    if (!compound_dim_ok(t->dim)) fail(MI_ERR_UNSUPPORTED, "dim %u: the paged search is built for dim in {128, 256, 512, 768, 1024}", t->dim);
    if (among) knn_filter_rows(t, among, n_among);   // every id checked before anything runs
    if (cursor_is_id && !page_first_key(page_ids(t), after_dist, after_id, &first_key))
        fail(MI_ERR_INVALID, "after_id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)after_id,
             (unsigned long long)t->base, (unsigned long long)t->rows);
    const uint64_t hi = page_hi(max_dist);
    const uint64_t n = among ? (uint64_t)t->n_flist : t->rows;
    if (n == 0) {
        page_pad(k, idx, dist, counts);
        return;
    }

    DeviceGuard g(t->device);
    hipStream_t s = knn_own_stream(t);
    const PageRecord rec = page_record(k);
    const uint32_t blocks = page_grid(n, t->n_cu, t->page_blocks), lists = blocks * 4;
    knn_reserve(t, (void**)&t->d_idx, &t->idx_cap, (rec.bytes + 7) / 8, sizeof(uint64_t));
    knn_reserve(t, (void**)&t->d_keys, &t->keys_cap, (size_t)PAGE_K_MAX, sizeof(uint64_t));
    if (k <= 64) knn_reserve(t, (void**)&t->d_cand, &t->cand_keys, (size_t)lists * k, sizeof(uint64_t));
    else knn_reserve(t, (void**)&t->d_keys32, &t->keys32_cap, (size_t)std::max<uint64_t>(n, t->cap), sizeof(uint32_t));
    // behind every write and search enqueued before this call, on whichever stream
    t->writes.begin(s);
    t->reads.begin(s);
    Settle settle{t, s};

    unsigned char* d_rec = reinterpret_cast<unsigned char*>(t->d_idx);
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(d_rec + rec.counts);
    HIP_CHECK(hipMemcpyAsync(t->d_q, q, (size_t)t->dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_counts, 0, 4 * sizeof(uint64_t), s));
    if (among) knn_filter_upload(t, s);
    const uint32_t* list = among ? t->d_flist : nullptr;
    const uint64_t* tomb = (among || t->dead.empty()) ? nullptr : t->d_tomb;
    uint64_t* cand = k <= 64 ? t->d_cand : nullptr;
    uint32_t* all_keys = k <= 64 ? nullptr : t->d_keys32;
    dispatch_nch(t->dim, [&](auto nch) {
        launch_scan<decltype(nch)::value>(t, blocks, s, n, list, tomb, first_key, hi, k, cand, all_keys, d_counts);
    });
    if (k <= 64) knn_reduce_lists64(t, lists, k, t->d_keys, s);
    else knn_select_keys32(t, n, k, t->d_keys, list, s);
    const IdMap map{t->base, t->cyc_block, t->cyc_n, t->cyc_rank};
    hipLaunchKernelGGL(knn_page_finish_kernel, dim3((k + 255) / 256), dim3(256), 0, s, t->d_keys, k, map,
                       reinterpret_cast<uint64_t*>(d_rec + rec.idx), reinterpret_cast<float*>(d_rec + rec.dist));
    HIP_CHECK(hipGetLastError());
    std::vector<unsigned char> h_rec(rec.bytes);
    HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec, rec.bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    page_unpack(h_rec.data(), k, idx, dist, counts);
}

}  // namespace mi

extern "C" {

int mi_knn_search_page(mi_knn* t, const float* q, uint32_t k, float after_dist, uint64_t after_id, float max_dist, const uint64_t* among,
                       uint64_t n_among, uint64_t* idx, float* dist, uint64_t counts[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = page_check_args(t, q, k, after_dist, after_id, max_dist, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        knn_search_page(t, q, k, true, after_dist, after_id, 0, max_dist, among, n_among, idx, dist, counts);
    });
}

}  // extern "C"
