// compound.hip — host side of mi_knn_search_compound: the k best rows under a score combined from several terms (near ALL /
// near ANY of the positive ones, not within a threshold of any negative one), exact, in one pass over the fp32 rows.
// The kernels, and why the combination is done on keys: compound_kernels.h.  The host-only rules: compound_host.h.
//
// One call: the padded term set goes up; knn_compound_scan_kernel leaves per-wave lists (k <= 64, reduced by the search's
// merge tree) or one score key per row (k > 64, the search's radix select); knn_compound_finish_kernel turns the k keys into
// one record (ids, scores, per-term distances, counts), which the host copies back in one piece.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "compound_host.h"
#include "compound_kernels.h"
#include "handles.h"
#include "two_stage.h"

using namespace mi;

namespace {

static_assert(COMPOUND_TERMS_MAX == (uint32_t)COMPOUND_MAX_TERMS, "the host's and the kernels' limit are one number");
static_assert(MI_COMPOUND_ALL == COMPOUND_ALL && MI_COMPOUND_ANY == COMPOUND_ANY, "the header's and the kernels' modes are one set");

template <int NCH>
void launch_scan(mi_knn* t, uint32_t padded, uint32_t blocks, hipStream_t s, uint64_t n, const uint32_t* list, const uint64_t* tomb,
                 const CompoundTerms& ct, uint32_t k, uint64_t* cand, uint32_t* all_keys, unsigned long long* counts) {
#define MI_CASE(NT)                                                                                                          \
    case NT:                                                                                                                 \
        hipLaunchKernelGGL((knn_compound_scan_kernel<NCH, NT>), dim3(blocks), dim3(256), 0, s, t->table, n, list, tomb, t->d_q, ct, k, \
                           cand, all_keys, counts);                                                                          \
        break;
    switch (padded) {
        MI_CASE(2) MI_CASE(4) MI_CASE(8)
        default: fail(MI_ERR_INVALID, "a term set of %u", padded);
    }
#undef MI_CASE
    HIP_CHECK(hipGetLastError());
}

}  // namespace

namespace mi {

// the call behind the C entry point (arguments checked by compound_check_args); throws Error
void knn_search_compound(mi_knn* t, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within, uint32_t n_neg,
                         uint32_t k, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, float* term_dist) {
    std::lock_guard<std::mutex> l(t->mu);
    if (!compound_dim_ok(t->dim)) fail(MI_ERR_UNSUPPORTED, "dim %u: the compound search is built for dim in {128, 256, 512, 768, 1024}", t->dim);
    if (among) knn_filter_rows(t, among, n_among);   // every id checked before anything runs
    for (uint64_t& v : t->compound_stats) v = 0;
    const uint32_t T = n_pos + n_neg;
    const uint64_t n = among ? (uint64_t)t->n_flist : t->rows;
    if (n == 0) {
        compound_pad(k, T, idx, dist, term_dist);
        return;
    }

    DeviceGuard g(t->device);
    hipStream_t s = knn_own_stream(t);
    const CompoundSet c = compound_set(pos, n_pos, neg, neg_within, n_neg, t->dim);
    const CompoundRecord rec = compound_record(k, T);
    const uint32_t blocks = compound_grid(n, t->n_cu, t->compound_blocks), lists = blocks * 4;
    knn_reserve(t, (void**)&t->d_idx, &t->idx_cap, (rec.bytes + 7) / 8, sizeof(uint64_t));
    knn_reserve(t, (void**)&t->d_keys, &t->keys_cap, (size_t)COMPOUND_K_MAX, sizeof(uint64_t));
    if (k <= 64) knn_reserve(t, (void**)&t->d_cand, &t->cand_keys, (size_t)lists * k, sizeof(uint64_t));
    else knn_reserve(t, (void**)&t->d_keys32, &t->keys32_cap, (size_t)std::max<uint64_t>(n, t->cap), sizeof(uint32_t));
    // behind every write and search enqueued before this call, on whichever stream
    t->writes.begin(s);
    t->reads.begin(s);
    Settle settle{t, s};

    unsigned char* d_rec = reinterpret_cast<unsigned char*>(t->d_idx);
    unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(d_rec + rec.stats);
    HIP_CHECK(hipMemcpyAsync(t->d_q, c.terms.data(), c.terms.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(uint64_t), s));
    if (among) knn_filter_upload(t, s);
    const uint32_t* list = among ? t->d_flist : nullptr;
    const uint64_t* tomb = (among || t->dead.empty()) ? nullptr : t->d_tomb;
    CompoundTerms ct;
    ct.neg_mask = c.neg_mask;
    ct.mode = mode;
    for (uint32_t u = 0; u < COMPOUND_TERMS_MAX; ++u) ct.within[u] = c.within[u];
    uint64_t* cand = k <= 64 ? t->d_cand : nullptr;
    uint32_t* all_keys = k <= 64 ? nullptr : t->d_keys32;
    dispatch_nch(t->dim, [&](auto nch) {
        launch_scan<decltype(nch)::value>(t, c.padded, blocks, s, n, list, tomb, ct, k, cand, all_keys, d_stats);
    });
    if (k <= 64) knn_reduce_lists64(t, lists, k, t->d_keys, s);
    else knn_select_keys32(t, n, k, t->d_keys, list, s);
    const IdMap map{t->base, t->cyc_block, t->cyc_n, t->cyc_rank};
    float* d_term = term_dist ? reinterpret_cast<float*>(d_rec + rec.term_dist) : nullptr;
    dispatch_nch(t->dim, [&](auto nch) {
        hipLaunchKernelGGL((knn_compound_finish_kernel<decltype(nch)::value>), dim3(group16_blocks(t, (uint64_t)k * (term_dist ? T : 1))), dim3(256),
                           0, s, t->table, t->d_keys, k, t->d_q, T, map, reinterpret_cast<uint64_t*>(d_rec + rec.idx),
                           reinterpret_cast<float*>(d_rec + rec.dist), d_term, d_stats);
    });
    HIP_CHECK(hipGetLastError());
    std::vector<unsigned char> h_rec(rec.bytes);
    HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec, term_dist ? rec.bytes : rec.term_dist, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t st[4];
    compound_unpack(h_rec.data(), k, T, idx, dist, term_dist, st);
    t->compound_stats[0] = n;
    t->compound_stats[1] = st[0];
    t->compound_stats[2] = st[1];
    t->compound_stats[3] = st[3];
}

}  // namespace mi

extern "C" {

int mi_knn_search_compound(mi_knn* t, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* neg_within, uint32_t n_neg,
                           uint32_t k, const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, float* term_dist) {
    return guarded([&] {
        const char* why = "";
        const int bad = compound_check_args(t, pos, n_pos, mode, neg, neg_within, n_neg, k, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (n_pos %u, n_neg %u, mode %d, k %u)", why, n_pos, n_neg, mode, k);
        knn_search_compound(t, pos, n_pos, mode, neg, neg_within, n_neg, k, among, n_among, idx, dist, term_dist);
    });
}

int mi_knn_search_compound_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->compound_stats[i];
    });
}

}  // extern "C"
