// where.hip — the table's attribute columns (mi_knn_set_attrs / get_attrs) and the predicate calls: mi_knn_count_where,
// mi_knn_rows_where, mi_knn_search_where.  A predicate over tags, stamp, the deletion bitmap and the group column becomes, on
// the device, the ascending list of qualifying rows in t->d_flist — what mi_knn_search_filtered builds on the host from an
// id list and uploads — and the search behind it is that call's own (knn_filtered_many).  The kernels: where_kernels.h.  The
// host-only rules: where_host.h.
//
// One call: where_count_kernel, where_offsets_kernel, an 8-byte copy of the total to a pinned word and one wait for it (the
// host needs n to size the list and to choose the grid and the selection path, as filtered_one does), where_emit_kernel.
#include <algorithm>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "scan_call.h"
#include "where_host.h"
#include "where_kernels.h"

using namespace mi;

namespace {

// the count and offsets passes on s, and the wait for their total: the qualifying rows.  Leaves the chunk offsets in
// t->d_wcounts + 2.  t->mu held, device selected, s ordered behind the handle's writes
uint64_t where_total(mi_knn* t, const mi_knn_where& w, hipStream_t s) {
    if (t->rows == 0 || where_never(w, t->d_groups != nullptr)) return 0;
    const uint32_t chunk = where_chunk_rows(t->where_chunk), chunks = where_chunks(t->rows, chunk);
    t->d_wcounts.reserve(t->reads, (size_t)chunks + 2);
    t->h_wtotal.reserve(sizeof(uint64_t));
    const unsigned long long* tomb = t->dead.empty() ? nullptr : reinterpret_cast<const unsigned long long*>(t->d_tomb.p);
    hipLaunchKernelGGL(where_count_kernel, dim3(chunks), dim3(WHERE_THREADS), 0, s, pred_of(w),
                       reinterpret_cast<const unsigned long long*>(t->d_tags.p), reinterpret_cast<const long long*>(t->d_stamps.p),
                       t->d_groups, tomb, t->rows, chunk, t->d_wcounts + 2);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(where_offsets_kernel, dim3(1), dim3(WHERE_SCAN_THREADS), 0, s, t->d_wcounts + 2, chunks,
                       reinterpret_cast<unsigned long long*>(t->d_wcounts.p));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(t->h_wtotal.p, t->d_wcounts, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return *t->h_wtotal.as<uint64_t>();
}

// ... and the emit pass: the rows into t->d_flist (room made first: the total is known), n_flist = their number
void where_list(mi_knn* t, const mi_knn_where& w, hipStream_t s) {
    const uint64_t total = where_total(t, w, s);
    t->n_flist = (size_t)total;
    if (total == 0) return;
    t->d_flist.reserve(t->reads, (size_t)total);
    const uint32_t chunk = where_chunk_rows(t->where_chunk), chunks = where_chunks(t->rows, chunk);
    const unsigned long long* tomb = t->dead.empty() ? nullptr : reinterpret_cast<const unsigned long long*>(t->d_tomb.p);
    hipLaunchKernelGGL(where_emit_kernel, dim3(chunks), dim3(WHERE_THREADS), 0, s, pred_of(w),
                       reinterpret_cast<const unsigned long long*>(t->d_tags.p), reinterpret_cast<const long long*>(t->d_stamps.p),
                       t->d_groups, tomb, t->rows, chunk, t->d_wcounts + 2, t->d_flist);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

namespace mi {

void knn_filter_where(mi_knn* t, const mi_knn_where* w, hipStream_t s) { where_list(t, *w, s); }

}  // namespace mi

extern "C" {

int mi_knn_set_attrs(mi_knn* t, const uint64_t* ids, uint64_t n, const uint64_t* tags, const int64_t* stamps) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_attrs_args(t, ids, n, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        if (n == 0 || (!tags && !stamps)) return;
        std::lock_guard<std::mutex> l(t->mu);
        const std::vector<uint32_t> rows = knn_local_rows(t, ids, n);   // every id checked before anything is written
        TableCall call(t);
        knn_attrs_fit(t);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t r = rows[(size_t)i];
            if (tags) t->d_tags.slot((size_t)t->rows, r) = tags[i];
            if (stamps) t->d_stamps.slot((size_t)t->rows, r) = stamps[i];
        }
        upload_span(call, rows, {{tags ? t->d_tags.p : nullptr, t->d_tags.host.data(), sizeof(uint64_t)},
                                 {stamps ? t->d_stamps.p : nullptr, t->d_stamps.host.data(), sizeof(int64_t)}});
    });
}

int mi_knn_get_attrs(mi_knn* t, const uint64_t* ids, uint64_t n, uint64_t* tags, int64_t* stamps) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_attrs_args(t, ids, n, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        if (n == 0) return;
        std::lock_guard<std::mutex> l(t->mu);
        const std::vector<uint32_t> rows = knn_local_rows(t, ids, n);
        for (uint64_t i = 0; i < n; ++i) {   // rows appended since the last set hold the defaults
            const uint32_t r = rows[(size_t)i];
            if (tags) tags[i] = t->d_tags.get(r);
            if (stamps) stamps[i] = t->d_stamps.get(r);
        }
    });
}

int mi_knn_count_where(mi_knn* t, const mi_knn_where* w, uint64_t* count) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_rows_args(t, w, nullptr, 0, count, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        std::lock_guard<std::mutex> l(t->mu);
        TableCall call(t);
        *count = where_total(t, *w, call.s);
    });
}

int mi_knn_rows_where(mi_knn* t, const mi_knn_where* w, uint64_t* ids, uint64_t cap, uint64_t* count) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_rows_args(t, w, ids, cap, count, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        std::lock_guard<std::mutex> l(t->mu);
        TableCall call(t);
        hipStream_t s = call.s;
        where_list(t, *w, s);
        *count = t->n_flist;
        const size_t take = (size_t)std::min<uint64_t>(cap, t->n_flist);
        if (take == 0) return;
        std::vector<uint32_t> rows(take);
        HIP_CHECK(hipMemcpyAsync(rows.data(), t->d_flist, take * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // a table's ids ascend with its local rows (a shard's too: block-cyclic placement keeps the order)
        const IdMap map = knn_id_map(t);
        for (size_t i = 0; i < take; ++i) ids[i] = id_of_local(map, rows[i]);
    });
}

// mi_knn_search_filtered with the list built on the device: the same grouping of the queries, the same kernels behind
int mi_knn_search_where(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w, uint64_t* idx, float* dist,
                        uint64_t* matched) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_search_args(t, q, nq, k, w, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        std::lock_guard<std::mutex> l(t->mu);
        TableCall call(t);
        hipStream_t s = call.s;
        constexpr uint32_t GROUP = 16;
        t->d_idx.reserve(t->reads, (size_t)GROUP * k);
        t->d_dist.reserve(t->reads, (size_t)GROUP * k);
        where_list(t, *w, s);
        if (matched) *matched = t->n_flist;
        for (uint32_t u0 = 0; u0 < nq; u0 += GROUP) {
            const uint32_t ng = std::min(GROUP, nq - u0);
            HIP_CHECK(hipMemcpyAsync(t->d_q, q + (size_t)u0 * t->dim, (size_t)ng * t->dim * sizeof(float), hipMemcpyHostToDevice, s));
            knn_filtered_many(t, t->d_q, ng, k, t->d_idx, t->d_dist, s);
            HIP_CHECK(hipMemcpyAsync(idx + (size_t)u0 * k, t->d_idx, (size_t)ng * k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(dist + (size_t)u0 * k, t->d_dist, (size_t)ng * k * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
    });
}

}  // extern "C"
