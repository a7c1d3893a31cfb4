// diverse.hip — host side of mi_knn_search_diverse: the k best results of a search with near-duplicates collapsed, and how
// many look-alikes stand behind each.  The kernels, and why positions in the gathered copy follow id order: diverse_kernels.h.
//
// One call: the search (plain or filtered) leaves its `pool` entries on the device; diverse_pool_kernel compacts them and
// gathers their rows; the host reads P (round trip 1); mirror_rows + join_tiles_kernel + diverse_rescore_kernel fill the
// conflict matrix through rect_stages (which reads a candidate count back per launch, as the join does);
// diverse_select_kernel walks it and writes one record, which the host copies back (round trip 2).
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "diverse_host.h"
#include "diverse_kernels.h"
#include "handles.h"
#include "join_kernels.h"
#include "two_stage.h"

using namespace mi;

namespace {

static_assert(DIVERSE_MAX_POOL == DIV_MAX_POOL, "the host's and the kernels' limit are one number");

// one allocation of a Scratch cut into aligned pieces
struct Carve {
    unsigned char* p = nullptr;
    size_t at = 0;
    size_t reserve(size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; }
    template <class T> T* ptr(size_t off) const { return reinterpret_cast<T*>(p + off); }
};

struct Diverse {
    mi_knn* t;
    hipStream_t s;
    uint32_t P, n_blocks, cand_cap;
    float min_gap, c;
    const float* copy;
    const uint16_t* mirror = nullptr;
    const float* xx = nullptr;
    const uint32_t* rank_of_pos;
    uint2* d_cand;
    unsigned long long* d_count;
    unsigned long long* d_conflict;
    uint32_t* d_n_conflicts;
    uint64_t candidates = 0;

    // the stages for rect_stages (two_stage.h): the join's tiles on or above the diagonal over the gathered copy (no deleted
    // rows in it: the search never returns one, so no tombstones), every candidate decided by diverse_rescore_kernel
    template <int NCH>
    void run() {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) -> unsigned long long {
            c0 = std::max(c0, r0);
            if (c0 >= c1) return 0;
            static DevOnce once;
            allow_lds_once(once, join_tiles_kernel<NCH>, JOIN_LDS);
            HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL((join_tiles_kernel<NCH>), dim3(c1 - c0, r1 - r0), dim3(256), JOIN_LDS, s, mirror, xx, (const uint64_t*)nullptr,
                               P, 0u, r0, c0, c, cand_cap, d_cand, d_count);
            HIP_CHECK(hipGetLastError());
            return read_count(d_count, s);
        };
        auto stage2 = [&](uint32_t C) {
            candidates += C;
            hipLaunchKernelGGL((diverse_rescore_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, copy, d_cand, C, min_gap,
                               rank_of_pos, d_conflict, d_n_conflicts);
            HIP_CHECK(hipGetLastError());
        };
        rect_stages(0, n_blocks, 0, n_blocks, cand_cap, nullptr, stage1, stage2);
    }
};

}  // namespace

extern "C" {

int mi_knn_search_diverse(mi_knn* t, const float* q, uint32_t k, uint32_t pool, float min_gap, const uint64_t* among, uint64_t n_among,
                          uint64_t* idx, float* dist, uint32_t* hidden, uint32_t* rep, uint32_t* n_kept) {
    return guarded([&] {
        const char* why = "";
        const int bad = diverse_check_args(t, q, k, pool, min_gap, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u, pool %u, min_gap %g)", why, k, pool, (double)min_gap);
        std::lock_guard<std::mutex> l(t->mu);
        for (uint64_t& v : t->diverse_stats) v = 0;
        if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "not offered on a shard of a sharded table");
        check_mirror_dim(t->dim, "the diverse search's");
        if (t->rows > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "a shard holds at most 2^32-1 rows");
        for (uint64_t i = 0; i < n_among; ++i)   // every id checked before anything runs
            if (among[i] < t->base || among[i] - t->base >= t->rows)
                fail(MI_ERR_INVALID, "id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)among[i],
                     (unsigned long long)t->base, (unsigned long long)t->rows);
        if (t->rows == 0 || (among && n_among == 0)) {
            diverse_pad(k, pool, idx, dist, hidden, rep, n_kept);
            return;
        }

        Scratch scratch;
        TableCall call(t);
        hipStream_t s = call.s;

        const DiverseRecord rec = diverse_record(k, pool);
        Carve a;
        const size_t o_sidx = a.reserve((size_t)pool * sizeof(uint64_t)), o_sdist = a.reserve((size_t)pool * sizeof(float));
        const size_t o_pidx = a.reserve((size_t)pool * sizeof(uint64_t)), o_pdist = a.reserve((size_t)pool * sizeof(float));
        const size_t o_rank = a.reserve((size_t)pool * sizeof(uint32_t)), o_rec = a.reserve(rec.bytes);
        const size_t o_copy = a.reserve((size_t)pool * t->dim * sizeof(float));
        a.p = (unsigned char*)scratch.get(a.at);
        uint64_t* d_sidx = a.ptr<uint64_t>(o_sidx);
        float* d_sdist = a.ptr<float>(o_sdist);
        unsigned char* d_rec = a.ptr<unsigned char>(o_rec);
        uint32_t* d_state = reinterpret_cast<uint32_t*>(d_rec + rec.state);

        HIP_CHECK(hipMemcpyAsync(t->d_q, q, (size_t)t->dim * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_state, 0, 4 * sizeof(uint32_t), s));
        if (among) knn_search_filtered_many(t, t->d_q, 1, pool, among, n_among, d_sidx, d_sdist, s);
        else knn_search_one(t, t->d_q, pool, d_sidx, d_sdist, s);
        hipLaunchKernelGGL(diverse_pool_kernel, dim3((pool + DIV_PER_BLOCK - 1) / DIV_PER_BLOCK), dim3(256), 0, s, t->table, t->dim, t->rows,
                           t->base, d_sidx, d_sdist, pool, a.ptr<uint64_t>(o_pidx), a.ptr<float>(o_pdist), a.ptr<uint32_t>(o_rank),
                           a.ptr<float>(o_copy), d_state + 3);
        HIP_CHECK(hipGetLastError());
        uint32_t P = 0;
        HIP_CHECK(hipMemcpyAsync(&P, d_state + 3, sizeof P, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (P > pool) fail(MI_ERR_HIP, "the pool came back with %u of %u entries", P, pool);

        Diverse d;
        d.t = t; d.s = s; d.P = P;
        d.n_blocks = (P + TILE - 1) / TILE;
        d.min_gap = min_gap;
        d.c = 1.0f - (min_gap + eps2(t->dim));
        const uint64_t all_pairs = (uint64_t)P * (P - (P ? 1 : 0)) / 2;   // no launch can count more candidates than this
        d.cand_cap = (uint32_t)std::max<uint64_t>(TILE_CAP_MIN, std::min<uint64_t>(t->join_cap, all_pairs));
        const uint32_t m_rows = ((P + DIV_CHUNK - 1) / DIV_CHUNK) * DIV_CHUNK;
        Carve b;
        const size_t o_conf = b.reserve((size_t)m_rows * DIV_WORDS * sizeof(unsigned long long));
        const size_t o_mirror = b.reserve((size_t)P * t->dim * sizeof(uint16_t)), o_xx = b.reserve((size_t)P * sizeof(float));
        const size_t o_cand = b.reserve((size_t)d.cand_cap * sizeof(uint2)), o_count = b.reserve(sizeof(unsigned long long));
        b.p = (unsigned char*)scratch.get(b.at);
        d.d_conflict = b.ptr<unsigned long long>(o_conf);
        d.copy = a.ptr<float>(o_copy);
        d.rank_of_pos = a.ptr<uint32_t>(o_rank);
        d.d_cand = b.ptr<uint2>(o_cand);
        d.d_count = b.ptr<unsigned long long>(o_count);
        d.d_n_conflicts = d_state + 2;
        if (m_rows) HIP_CHECK(hipMemsetAsync(d.d_conflict, 0, (size_t)m_rows * DIV_WORDS * sizeof(unsigned long long), s));
        if (P >= 2) {
            mirror_rows(t, s, d.copy, 0, P, b.ptr<uint16_t>(o_mirror), b.ptr<float>(o_xx));
            d.mirror = b.ptr<uint16_t>(o_mirror);
            d.xx = b.ptr<float>(o_xx);
            dispatch_nch(t->dim, [&](auto nch) { d.template run<decltype(nch)::value>(); });
        }
        hipLaunchKernelGGL(diverse_select_kernel, dim3(1), dim3(256), 0, s, d.d_conflict, d_state + 3, a.ptr<uint64_t>(o_pidx),
                           a.ptr<float>(o_pdist), k, pool, reinterpret_cast<uint64_t*>(d_rec + rec.idx), reinterpret_cast<float*>(d_rec + rec.dist),
                           reinterpret_cast<uint32_t*>(d_rec + rec.hidden), reinterpret_cast<uint32_t*>(d_rec + rec.rep), d_state);
        HIP_CHECK(hipGetLastError());
        std::vector<unsigned char> h_rec(rec.bytes);
        HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec, rec.bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        uint32_t state[4];
        diverse_unpack(h_rec.data(), k, pool, idx, dist, hidden, rep, n_kept, state);
        t->diverse_stats[0] = P;
        t->diverse_stats[1] = d.candidates;
        t->diverse_stats[2] = state[2];
        t->diverse_stats[3] = state[1];
    });
}

int mi_knn_search_diverse_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->diverse_stats[i];
    });
}

}  // extern "C"
