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
#include "compound_host.h"
#include "grouped_host.h"
#include "grouped_kernels.h"
#include "handles.h"
#include "two_stage.h"

using namespace mi;

namespace {

PageIds ids_of(const mi_knn* t) { return PageIds{t->base, t->rows, t->cyc_block, t->cyc_n, t->cyc_rank}; }

// ids (nullable: the first n rows) -> local rows, every one checked; MI_ERR_INVALID names the first that is no row
std::vector<uint32_t> local_rows(const mi_knn* t, const uint64_t* ids, uint64_t n) {
    if (!ids && n > t->rows) fail(MI_ERR_INVALID, "%llu rows asked of a table of %llu", (unsigned long long)n, (unsigned long long)t->rows);
    std::vector<uint32_t> rows((size_t)n);
    const PageIds m = ids_of(t);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t local = i;
        if (ids && !page_local_of(m, ids[i], &local))
            fail(MI_ERR_INVALID, "id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)ids[i],
                 (unsigned long long)t->base, (unsigned long long)t->rows);
        rows[(size_t)i] = (uint32_t)local;
    }
    return rows;
}

}  // namespace

namespace mi {

// the call behind the C entry points (arguments checked by grouped_check_args); throws Error.  cnt_out (nullable): the
// per-group counts as the device holds them, [t->n_groups] — what the sharded call sums.
void knn_search_grouped(mi_knn* t, const float* q, uint32_t k, float max_dist, const uint64_t* among, uint64_t n_among, uint64_t* idx,
                        float* dist, uint32_t* group, uint64_t* members, uint64_t* facets, uint64_t cap_facets, uint64_t* totals,
                        std::vector<uint32_t>* cnt_out) {
    std::lock_guard<std::mutex> l(t->mu);
    if (!compound_dim_ok(t->dim)) fail(MI_ERR_UNSUPPORTED, "dim %u: the grouped search is built for dim in {128, 256, 512, 768, 1024}", t->dim);
    const uint32_t G = t->n_groups;
    if (facets && cap_facets < G) fail(MI_ERR_INVALID, "facets holds %llu entries, the table has %u groups", (unsigned long long)cap_facets, G);
    if (among) knn_filter_rows(t, among, n_among);   // every id checked before anything runs
    const uint64_t hi = page_hi(max_dist);
    const uint64_t n = among ? (uint64_t)t->n_flist : t->rows;
    t->gslots_valid = false;
    if (n == 0) {
        grouped_pad(k, idx, dist, group, members, totals);
        if (facets) std::fill(facets, facets + G, 0ull);
        if (cnt_out) cnt_out->assign(G, 0u);
        return;
    }

    DeviceGuard g(t->device);
    hipStream_t s = knn_own_stream(t);
    const GroupedRecord rec = grouped_record(k);
    const uint32_t blocks = grouped_grid(n, t->n_cu, t->group_blocks);
    knn_reserve(t, (void**)&t->d_idx, &t->idx_cap, (rec.bytes + 7) / 8, sizeof(uint64_t));
    knn_reserve(t, (void**)&t->d_keys, &t->keys_cap, (size_t)PAGE_K_MAX, sizeof(uint64_t));
    knn_reserve(t, (void**)&t->d_keys32, &t->keys32_cap, (size_t)std::max<uint64_t>(n, t->cap), sizeof(uint32_t));
    if (G) knn_reserve(t, (void**)&t->d_gslots, &t->gslots_cap, (size_t)G * 3, sizeof(uint32_t));
    // behind every write and search enqueued before this call, on whichever stream
    t->writes.begin(s);
    t->reads.begin(s);
    Settle settle{t, s};

    unsigned char* d_rec = reinterpret_cast<unsigned char*>(t->d_idx);
    unsigned long long* d_totals = reinterpret_cast<unsigned long long*>(d_rec + rec.totals);
    unsigned long long* d_best = reinterpret_cast<unsigned long long*>(t->d_gslots);   // [G] u64, then [G] u32
    uint32_t* d_cnt = t->d_gslots ? t->d_gslots + (size_t)G * 2 : nullptr;
    HIP_CHECK(hipMemcpyAsync(t->d_q, q, (size_t)t->dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_totals, 0, 4 * sizeof(uint64_t), s));
    if (G) {
        HIP_CHECK(hipMemsetAsync(d_best, 0xFF, (size_t)G * sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)G * sizeof(uint32_t), s));
    }
    if (among) knn_filter_upload(t, s);
    const uint32_t* list = among ? t->d_flist : nullptr;
    const uint64_t* tomb = (among || t->dead.empty()) ? nullptr : t->d_tomb;
    knn_page_scan_keys32(t, s, n, list, tomb, hi, k, t->d_keys32, d_totals);
    if (G) {
        // the scan counts nothing "before" (there is no cursor): totals[0] is free for the representatives
        if (grouped_use_lds(G, (uint32_t)t->group_lds_max))
            hipLaunchKernelGGL((group_reduce_kernel<1>), dim3(blocks), dim3(256), (size_t)G * GROUP_SLOT_BYTES, s, t->d_keys32, n, list,
                               t->d_groups, G, d_best, d_cnt);
        else
            hipLaunchKernelGGL((group_reduce_kernel<0>), dim3(blocks), dim3(256), 0, s, t->d_keys32, n, list, t->d_groups, G, d_best, d_cnt);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(group_mark_kernel, dim3(blocks), dim3(256), 0, s, t->d_keys32, n, list, t->d_groups, G, d_best, d_totals);
        HIP_CHECK(hipGetLastError());
    }
    knn_select_keys32(t, n, k, t->d_keys, list, s);
    const IdMap map{t->base, t->cyc_block, t->cyc_n, t->cyc_rank};
    hipLaunchKernelGGL(group_finish_kernel, dim3((k + 255) / 256), dim3(256), 0, s, t->d_keys, k, map, G ? t->d_groups : nullptr, G, d_cnt,
                       reinterpret_cast<uint64_t*>(d_rec + rec.idx), reinterpret_cast<uint64_t*>(d_rec + rec.members),
                       reinterpret_cast<float*>(d_rec + rec.dist), reinterpret_cast<uint32_t*>(d_rec + rec.group));
    HIP_CHECK(hipGetLastError());
    std::vector<unsigned char> h_rec(rec.bytes);
    std::vector<uint32_t> h_cnt;
    HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec, rec.bytes, hipMemcpyDeviceToHost, s));
    if (G && (facets || cnt_out)) {
        h_cnt.resize(G);
        HIP_CHECK(hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)G * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t tot[4];
    grouped_unpack(h_rec.data(), k, idx, dist, group, members, tot);
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
    DeviceGuard g(t->device);
    hipStream_t s = knn_own_stream(t);
    knn_reserve(t, (void**)&t->d_gwin, &t->gwin_cap, (size_t)2 * PAGE_K_MAX, sizeof(uint32_t));
    t->writes.begin(s);
    t->reads.begin(s);
    Settle settle{t, s};
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
        const std::vector<uint32_t> rows = local_rows(t, ids, n);   // every id checked before anything is written
        DeviceGuard g(t->device);
        hipStream_t s = knn_own_stream(t);
        knn_groups_fit(t);
        if (t->h_groups.size() < t->rows) t->h_groups.resize((size_t)t->rows, MI_KNN_NO_GROUP);
        uint32_t lo = 0xFFFFFFFFu, hi = 0;
        for (uint64_t i = 0; i < n; ++i) {
            uint32_t& slot = t->h_groups[rows[(size_t)i]];
            t->n_grouped += (groups[i] != MI_KNN_NO_GROUP) - (slot != MI_KNN_NO_GROUP);
            slot = groups[i];
            if (groups[i] != MI_KNN_NO_GROUP) t->n_groups = std::max(t->n_groups, groups[i] + 1);
            lo = std::min(lo, rows[(size_t)i]);
            hi = std::max(hi, rows[(size_t)i]);
        }
        // a write that changes what searches read: behind the searches enqueued before it, ahead of every later one.  The
        // span of rows the call names goes up in one copy (the host holds the column too).
        t->writes.begin(s);
        t->reads.begin(s);
        HIP_CHECK(hipMemcpyAsync(t->d_groups + lo, t->h_groups.data() + lo, (size_t)(hi - lo + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        t->writes.end(s);
        HIP_CHECK(hipStreamSynchronize(s));
        ++t->groups_epoch;
    });
}

int mi_knn_get_groups(mi_knn* t, const uint64_t* ids, uint64_t n, uint32_t* groups) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        if (!groups) fail(MI_ERR_INVALID, "groups is null");
        std::lock_guard<std::mutex> l(t->mu);
        const std::vector<uint32_t> rows = local_rows(t, ids, n);
        for (uint64_t i = 0; i < n; ++i)   // rows appended since the last set hold no group
            groups[i] = rows[(size_t)i] < t->h_groups.size() ? t->h_groups[rows[(size_t)i]] : MI_KNN_NO_GROUP;
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
