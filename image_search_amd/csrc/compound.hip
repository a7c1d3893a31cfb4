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
#include "scan_call.h"
#include "two_stage.h"

using namespace mi;

namespace {

static_assert(COMPOUND_K_MAX <= SCAN_K_MAX, "the shared selection delivers every k the call accepts");
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
    check_scan_dim(t->dim, "the compound search");
    const ScanFrom from = among ? SCAN_HOST_IDS : SCAN_TABLE;
    if (among) knn_filter_rows(t, among, n_among);   // every id checked before anything runs
    for (uint64_t& v : t->compound_stats) v = 0;
    const uint32_t T = n_pos + n_neg;
    const uint64_t n = scan_count(t, from);
    if (n == 0) {
        compound_pad(k, T, idx, dist, term_dist);
        return;
    }

    TableCall call(t);
    hipStream_t s = call.s;
    const CompoundSet c = compound_set(pos, n_pos, neg, neg_within, n_neg, t->dim);
    const CompoundRecord rec = compound_record(k, T);
    const uint32_t blocks = scan_grid(n, t->n_cu, t->compound_blocks, COMPOUND_BLOCKS_PER_CU);
    unsigned char* d_rec = scan_record(t, rec.bytes);
    const ScanSelect sel = scan_select_reserve(t, n, k, blocks * 4);

    unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(d_rec + rec.stats);
    HIP_CHECK(hipMemcpyAsync(t->d_q, c.terms.data(), c.terms.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(uint64_t), s));
    const ScanSet cs = scan_set(t, s, from);
    CompoundTerms ct;
    ct.neg_mask = c.neg_mask;
    ct.mode = mode;
    for (uint32_t u = 0; u < COMPOUND_TERMS_MAX; ++u) ct.within[u] = c.within[u];
    dispatch_nch(t->dim, [&](auto nch) {
        launch_scan<decltype(nch)::value>(t, c.padded, blocks, s, n, cs.list, cs.tomb, ct, k, sel.cand, sel.all_keys, d_stats);
    });
    scan_select(t, sel, cs.list, s);
    float* d_term = term_dist ? reinterpret_cast<float*>(d_rec + rec.term_dist) : nullptr;
    dispatch_nch(t->dim, [&](auto nch) {
        hipLaunchKernelGGL((knn_compound_finish_kernel<decltype(nch)::value>), dim3(group16_blocks(t, (uint64_t)k * (term_dist ? T : 1))), dim3(256),
                           0, s, t->table, t->d_keys, k, t->d_q, T, knn_id_map(t), reinterpret_cast<uint64_t*>(d_rec + rec.idx),
                           reinterpret_cast<float*>(d_rec + rec.dist), d_term, d_stats);
    });
    HIP_CHECK(hipGetLastError());
    uint64_t st[4];
    compound_unpack(scan_record_fetch(d_rec, term_dist ? rec.bytes : rec.term_dist, s).data(), k, T, idx, dist, term_dist, st);
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
