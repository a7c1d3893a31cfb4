// grouped.hip — the table's group column (mi_knn_set_groups / get_groups / groups_info) and mi_knn_search_grouped: the best
// in-window row of every group, the k best of those, how many in-window rows each group has, exact, in one pass over the fp32
// rows plus three short passes over 12 bytes per row.  The kernels, and why the reduction is not fused into the scan:
// grouped_kernels.h.  The host-only rules: grouped_host.h.
//
// One call: the query goes up; knn_page_scan_kernel<NCH, 1> (no cursor) leaves one distance key per row or list entry and the
// window counts; group_reduce_kernel builds best[g] / cnt[g]; group_mark_kernel takes every non-representative out of the keys
// and counts the representatives; the search's radix select picks the k smallest; group_finish_kernel turns them into one
// record beside the totals, and the host copies that record back in one piece (the per-group counts follow only when the
// caller asks for facets).
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "grouped_host.h"
#include "grouped_kernels.h"
#include "handles.h"
#include "scan_call.h"
#include "two_stage.h"

using namespace mi;

namespace mi {

// the call behind the C entry points (arguments checked by grouped_check_args); throws Error.  cnt_out (nullable): the
// per-group counts as the device holds them, [t->n_groups] — what the sharded call sums.
void knn_search_grouped(mi_knn* t, const float* q, uint32_t k, float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx,
                        float* dist, uint32_t* group, uint64_t* members, uint64_t* facets, uint64_t cap_facets, uint64_t* totals,
                        std::vector<uint32_t>* cnt_out) {
    std::lock_guard<std::mutex> l(t->mu);
    check_scan_dim(t->dim, "the grouped search");
    const uint32_t G = t->n_groups;
    if (facets && cap_facets < G) fail(MI_ERR_INVALID, "facets holds %llu entries, the table has %u groups", (unsigned long long)cap_facets, G);
    const ScanFrom from = among ? SCAN_HOST_IDS : SCAN_TABLE;
    if (among) knn_filter_rows(t, among, n_among);   // every id checked before anything runs
    const uint64_t hi = page_hi(max_dist);
    const uint64_t n = scan_count(t, from);
    t->gslots_valid = false;
    if (n == 0) {
        grouped_pad(k, idx, dist, group, members, totals);
        if (facets) std::fill(facets, facets + G, 0ull);
        if (cnt_out) cnt_out->assign(G, 0u);
        return;
    }

    TableCall call(t);
    hipStream_t s = call.s;
    const GroupedRecord rec = grouped_record(k);
    const uint32_t blocks = grouped_grid(n, t->n_cu, t->group_blocks);
    unsigned char* d_rec = scan_record(t, rec.bytes);
    uint32_t* keys32 = scan_keys32(t, n);
    if (G) t->d_gslots.reserve(t->reads, (size_t)G * 3);

    unsigned long long* d_totals = reinterpret_cast<unsigned long long*>(d_rec + rec.totals);
    unsigned long long* d_best = reinterpret_cast<unsigned long long*>(t->d_gslots.p);   // [G] u64, then [G] u32
    uint32_t* d_cnt = t->d_gslots ? t->d_gslots + (size_t)G * 2 : nullptr;
    HIP_CHECK(hipMemcpyAsync(t->d_q, q, (size_t)t->dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_totals, 0, 4 * sizeof(uint64_t), s));
    if (G) {
        HIP_CHECK(hipMemsetAsync(d_best, 0xFF, (size_t)G * sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)G * sizeof(uint32_t), s));
    }
    const ScanSet c = scan_set(t, s, from);
    knn_page_scan_keys32(t, s, n, c.list, c.tomb, hi, k, keys32, d_totals);
    if (G) {
        // the scan counts nothing "before" (there is no cursor): totals[0] is free for the representatives
        if (grouped_use_lds(G, (uint32_t)t->group_lds_max))
            hipLaunchKernelGGL((group_reduce_kernel<1>), dim3(blocks), dim3(256), (size_t)G * GROUP_SLOT_BYTES, s, keys32, n, c.list,
                               t->d_groups, G, d_best, d_cnt);
        else
            hipLaunchKernelGGL((group_reduce_kernel<0>), dim3(blocks), dim3(256), 0, s, keys32, n, c.list, t->d_groups, G, d_best, d_cnt);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(group_mark_kernel, dim3(blocks), dim3(256), 0, s, keys32, n, c.list, t->d_groups, G, d_best, d_totals);
        HIP_CHECK(hipGetLastError());
    }
    knn_select_keys32(t, n, k, t->d_keys, c.list, s);
    hipLaunchKernelGGL(group_finish_kernel, dim3((k + 255) / 256), dim3(256), 0, s, t->d_keys, k, knn_id_map(t), G ? t->d_groups : nullptr, G,
                       d_cnt, reinterpret_cast<uint64_t*>(d_rec + rec.idx), reinterpret_cast<uint64_t*>(d_rec + rec.members),
                       reinterpret_cast<float*>(d_rec + rec.dist), reinterpret_cast<uint32_t*>(d_rec + rec.group));
    HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> h_cnt;   // the per-group counts go back in front of the record, under its one wait
    if (G && (facets || cnt_out)) {
        h_cnt.resize(G);
        HIP_CHECK(hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)G * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    uint64_t tot[4];
    grouped_unpack(scan_record_fetch(d_rec, rec.bytes, s).data(), k, idx, dist, group, members, tot);
    if (!G) tot[0] = tot[1];   // no group anywhere: every row of the window stands for itself
    if (totals) std::copy(tot, tot + 4, totals);
    if (facets) std::copy(h_cnt.begin(), h_cnt.end(), facets);
    if (cnt_out) cnt_out->swap(h_cnt);
    t->gslots_valid = G != 0;
    t->gslots_groups = G;
}

// out[j] = this table's count, from its LAST grouped search, of group[j] (0 for MI_KNN_NO_GROUP and for a group it does not
// know); a table whose last grouped search had no candidate answers zeros.  takes t->mu
void knn_grouped_members(mi_knn* t, const uint32_t* group, uint32_t k, uint32_t* out) {
    std::lock_guard<std::mutex> l(t->mu);
    std::fill(out, out + k, 0u);
    if (!t->gslots_valid || k == 0) return;
    TableCall call(t);
    hipStream_t s = call.s;
    t->d_gwin.reserve(t->reads, (size_t)2 * PAGE_K_MAX);
    const uint32_t G = t->gslots_groups;
    HIP_CHECK(hipMemcpyAsync(t->d_gwin, group, (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(group_gather_kernel, dim3((k + 255) / 256), dim3(256), 0, s, t->d_gwin, k, t->d_gslots + (size_t)G * 2, G,
                       t->d_gwin + PAGE_K_MAX);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, t->d_gwin + PAGE_K_MAX, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace mi

extern "C" {

int mi_knn_set_groups(mi_knn* t, const uint64_t* ids, uint64_t n, const uint32_t* groups) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        if (!groups) fail(MI_ERR_INVALID, "groups is null");
        const uint64_t bad = grouped_first_bad(groups, n);
        if (bad < n) fail(MI_ERR_INVALID, "group id %u (entry %llu) is neither below 2^24 nor MI_KNN_NO_GROUP", groups[bad], (unsigned long long)bad);
        std::lock_guard<std::mutex> l(t->mu);
        const std::vector<uint32_t> rows = knn_local_rows(t, ids, n);   // every id checked before anything is written
        TableCall call(t);
        knn_groups_fit(t);
        for (uint64_t i = 0; i < n; ++i) {
            uint32_t& slot = t->d_groups.slot((size_t)t->rows, rows[(size_t)i]);
            t->n_grouped += (groups[i] != MI_KNN_NO_GROUP) - (slot != MI_KNN_NO_GROUP);
            slot = groups[i];
            if (groups[i] != MI_KNN_NO_GROUP) t->n_groups = std::max(t->n_groups, groups[i] + 1);
        }
        upload_span(call, rows, {{t->d_groups.p, t->d_groups.host.data(), sizeof(uint32_t)}});
        ++t->groups_epoch;
    });
}

int mi_knn_get_groups(mi_knn* t, const uint64_t* ids, uint64_t n, uint32_t* groups) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        if (!groups) fail(MI_ERR_INVALID, "groups is null");
        std::lock_guard<std::mutex> l(t->mu);
        const std::vector<uint32_t> rows = knn_local_rows(t, ids, n);
        for (uint64_t i = 0; i < n; ++i) groups[i] = t->d_groups.get(rows[(size_t)i]);   // rows appended since the last set hold no group
    });
}

int mi_knn_groups_info(mi_knn* t, uint64_t info[2]) {
    return guarded([&] {
        if (!t || !info) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        info[0] = t->n_groups;
        info[1] = t->n_grouped;
    });
}

int mi_knn_search_grouped(mi_knn* t, const float* q, uint32_t k, float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx,
                          float* dist, uint32_t* group, uint64_t* members, uint64_t* facets, uint64_t cap_facets, uint64_t totals[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = grouped_check_args(t, q, k, max_dist, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        knn_search_grouped(t, q, k, max_dist, among, n_among, idx, dist, group, members, facets, cap_facets, totals, nullptr);
    });
}

}  // extern "C"
