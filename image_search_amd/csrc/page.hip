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
#include "handles.h"
#include "page_host.h"
#include "page_kernels.h"
#include "scan_call.h"
#include "two_stage.h"

using namespace mi;

namespace {

static_assert(PAGE_K_MAX <= SCAN_K_MAX, "the shared selection delivers every k the call accepts");

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

}  // namespace

namespace mi {

// the scan without a cursor in its one-key-per-row form, for the grouped search (grouped.hip): keys32 [n] = the distance key of
// every row or list entry, 0xFFFFFFFF outside the window [0, hi]; counts += {0, window, beyond, nan}.  t->mu held, device
// selected, the query in t->d_q
void knn_page_scan_keys32(mi_knn* t, hipStream_t s, uint64_t n, const uint32_t* list, const uint64_t* tomb, uint64_t hi, uint32_t k,
                          uint32_t* keys32, unsigned long long* counts) {
    const uint32_t blocks = scan_grid(n, t->n_cu, t->page_blocks, PAGE_BLOCKS_PER_CU);
    dispatch_nch(t->dim, [&](auto nch) { launch_scan<decltype(nch)::value>(t, blocks, s, n, list, tomb, 0, hi, k, nullptr, keys32, counts); });
}

// the call behind the C entry points (arguments checked by page_check_args); throws Error.  cursor_is_id: first_key is built
// here from (after_dist, after_id), which must name a row of t; otherwise the caller — the sharded call — hands first_key over.
void knn_search_page(mi_knn* t, const float* q, uint32_t k, bool cursor_is_id, float after_dist, uint64_t after_id, uint64_t first_key,
                     float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, uint64_t* counts) {
    std::lock_guard<std::mutex> l(t->mu);
    check_scan_dim(t->dim, "the paged search");
    const ScanFrom from = among ? SCAN_HOST_IDS : SCAN_TABLE;
    if (among) knn_filter_rows(t, among, n_among);   // every id checked before anything runs
    if (cursor_is_id && !page_first_key(knn_id_map(t), t->rows, after_dist, after_id, &first_key))
        fail(MI_ERR_INVALID, "after_id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)after_id,
             (unsigned long long)t->base, (unsigned long long)t->rows);
    const uint64_t hi = page_hi(max_dist);
    const uint64_t n = scan_count(t, from);
    if (n == 0) {
        page_pad(k, idx, dist, counts);
        return;
    }

    TableCall call(t);
    hipStream_t s = call.s;
    const PageRecord rec = page_record(k);
    const uint32_t blocks = scan_grid(n, t->n_cu, t->page_blocks, PAGE_BLOCKS_PER_CU);
    unsigned char* d_rec = scan_record(t, rec.bytes);
    const ScanSelect sel = scan_select_reserve(t, n, k, blocks * 4);

    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(d_rec + rec.counts);
    HIP_CHECK(hipMemcpyAsync(t->d_q, q, (size_t)t->dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_counts, 0, 4 * sizeof(uint64_t), s));
    const ScanSet c = scan_set(t, s, from);
    dispatch_nch(t->dim, [&](auto nch) {
        launch_scan<decltype(nch)::value>(t, blocks, s, n, c.list, c.tomb, first_key, hi, k, sel.cand, sel.all_keys, d_counts);
    });
    scan_select(t, sel, c.list, s);
    hipLaunchKernelGGL(knn_page_finish_kernel, dim3((k + 255) / 256), dim3(256), 0, s, t->d_keys, k, knn_id_map(t),
                       reinterpret_cast<uint64_t*>(d_rec + rec.idx), reinterpret_cast<float*>(d_rec + rec.dist));
    HIP_CHECK(hipGetLastError());
    page_unpack(scan_record_fetch(d_rec, rec.bytes, s).data(), k, idx, dist, counts);
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
