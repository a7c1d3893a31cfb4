// search_many.hip — host side of mi_knn_search_many (the k <= 16 nearest live rows for each of nq query vectors), of
// mi_knn_neighbors (the same with the table's own rows as the queries: a slice of the kNN graph) and of
// mi_knn_sharded_search_many.  The kernels and the superset argument: search_many_kernels.h.
//
// The queries are walked in strips of at most STRIP_TILES row tiles.  A strip owns all per-query state: its fp32 queries
// and their bf16 mirror (mi_knn_search_many; mi_knn_neighbors reads both where they lie), the threshold slots of stage 1
// (4 m bytes per query), the key slots of stage 2 (8 m bytes) and the unpacked results (12 k bytes).  With the candidate
// buffer ("join_cap" pairs of 8 bytes) that is the device workspace beyond the table's mirror: it does not grow with nq.
// Per strip: one threshold pass, then the emit pass in pieces of row tiles sized so that a piece's candidates fit the
// buffer (from the rate the previous piece saw); a piece that overflows is redone in halves, query tiles first, then
// column ranges — only its emit pass: the strip's thresholds stay valid for every piece.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "handles.h"
#include "search_many_kernels.h"

namespace mi {
void merge_lists(const uint64_t* idx_in, const float* dist_in, uint32_t lists, uint32_t k, uint64_t* idx, float* dist);   // core.hip
}

using namespace mi;
using namespace mi_search_many::mi_assign_multi::mi;

namespace {

constexpr uint32_t STRIP_TILES = 512;   // query tiles of a strip (65 536 queries)
constexpr uint32_t MAX_K = 16;
constexpr uint32_t MAX_SEGMENTS = 65535;   // grid.y

// device memory of one call, freed on every way out
struct Scratch {
    std::vector<void*> p;
    void* get(size_t bytes) {
        void* q = nullptr;
        HIP_CHECK(hipMalloc(&q, std::max<size_t>(bytes, 16)));
        p.push_back(q);
        return q;
    }
    ~Scratch() {
        for (void* q : p) (void)hipFree(q);
    }
};

// the table's own mirror grows with its capacity, keeping the rows mirrored so far (as assign_multi.hip)
void grow_keep(mi_knn* t, void** p, size_t* have, size_t want, size_t elem, size_t keep) {
    if (*have >= want) return;
    t->reads.sync();
    void* np_ = nullptr;
    HIP_CHECK(hipMalloc(&np_, want * elem));
    if (*p && keep) HIP_CHECK(hipMemcpy(np_, *p, std::min(keep, *have) * elem, hipMemcpyDeviceToDevice));
    if (*p) HIP_CHECK(hipFree(*p));
    *p = np_;
    *have = want;
}

template <int NCH>
void launch_mirror(hipStream_t s, int n_cu, const float* rows, uint64_t from, uint64_t end, uint16_t* mirror, float* xx) {
    const uint32_t mb = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((uint64_t)n_cu * 8, (end - from + 15) / 16));
    hipLaunchKernelGGL((knn_mirror_kernel<NCH>), dim3(mb), dim3(256), 0, s, rows, from, end, mirror, xx);
    HIP_CHECK(hipGetLastError());
}

void mirror_rows(mi_knn* t, hipStream_t s, const float* rows, uint64_t from, uint64_t end, uint16_t* mirror, float* xx) {
    switch (t->dim / 64) {
#define MI_CASE(NCH) case NCH: launch_mirror<NCH>(s, t->n_cu, rows, from, end, mirror, xx); break;
        MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
    }
}

// One call's state: the table's mirror (the columns), one strip's queries, slots and results on the device.
struct SearchMany {
    mi_knn* t = nullptr;
    hipStream_t s = nullptr;
    Scratch scratch;
    uint32_t n_cols = 0, m = 0, k = 0, n_cb = 0, cand_cap = 0, strip_rows = 0, sample = 1;
    bool self_drop = false;
    float thr = 0.0f;
    const uint16_t* mirror = nullptr;
    const float* xx = nullptr;
    const uint64_t* tomb = nullptr;
    // the strip under way: n_s queries, fp32 and mirrored; for mi_knn_neighbors query r is the table's local row q_local0 + r
    const float* qf = nullptr;
    const uint16_t* qm = nullptr;
    const float* qx = nullptr;
    const uint64_t* q_tomb = nullptr;
    uint32_t q_local0 = 0, n_s = 0;
    float* d_qf = nullptr;           // [strip rows][dim] (mi_knn_search_many)
    uint16_t* d_qm = nullptr;
    float* d_qx = nullptr;
    uint2* d_cand = nullptr;
    unsigned long long *d_count = nullptr, *d_hits = nullptr, *d_slot = nullptr;
    int* d_gslot = nullptr;          // [strip rows][m]: stage 1's thresholds
    uint64_t* d_idx = nullptr;       // [strip rows][k]
    float* d_dist = nullptr;
    uint64_t stats[4] = {0, 0, 0, 0};

    // segments of a launch over n_rt row tiles and n_i column tiles: "many_segments" or enough that the workgroups are
    // several times the machine's slots, a segment not shorter than four tiles
    uint32_t segments(uint32_t n_rt, uint32_t n_i) const {
        uint32_t v = t->many_segments > 0 ? (uint32_t)t->many_segments
                                          : std::min<uint32_t>(((uint32_t)t->n_cu * 16 + n_rt - 1) / n_rt, std::max(1u, n_i / 4));
        return std::max(1u, std::min({v, n_i, MAX_SEGMENTS}));
    }

    template <int NCH, bool EMIT>
    void tiles(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t step, uint32_t n_i) {
        static DevOnce once;
        constexpr int LDS = EMIT ? SMY_LDS_EMIT : SMY_LDS_THR;
        allow_lds_once(once, search_many_tiles_kernel<NCH, EMIT>, LDS);
        hipLaunchKernelGGL((search_many_tiles_kernel<NCH, EMIT>), dim3(br1 - br0, segments(br1 - br0, n_i)), dim3(256), LDS, s, qm, qx,
                           q_tomb, q_local0, n_s, mirror, xx, tomb, n_cols, m, br0, bc0, step, n_i, thr, d_gslot, cand_cap, d_cand,
                           d_count);
        HIP_CHECK(hipGetLastError());
        ++stats[2];
        stats[3] += (uint64_t)(br1 - br0) * n_i;
    }

    // the emit pass of query tiles [br0, br1) x column tiles [bc0, bc1), and stage 2 of what it found
    template <int NCH>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        if (bc0 >= bc1 || br0 >= br1) return;
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
        tiles<NCH, true>(br0, br1, bc0, 1, bc1 - bc0);
        unsigned long long n_cand = 0;
        HIP_CHECK(hipMemcpyAsync(&n_cand, d_count, sizeof n_cand, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (n_cand > cand_cap) {   // nothing is dropped and nothing rescored: the same ground again in two halves
            if (overflowed) *overflowed = true;
            if (br1 - br0 > 1) {
                const uint32_t mid = br0 + (br1 - br0) / 2;
                rect<NCH>(br0, mid, bc0, bc1, nullptr);
                rect<NCH>(mid, br1, bc0, bc1, nullptr);
            } else if (bc1 - bc0 > 1) {   // (the queries' slots of stage 2 live in d_slot: they join the column pieces)
                const uint32_t mid = bc0 + (bc1 - bc0) / 2;
                rect<NCH>(br0, br1, bc0, mid, nullptr);
                rect<NCH>(br0, br1, mid, bc1, nullptr);
            } else {
                fail(MI_ERR_INVALID, "one tile reported %llu candidates (the buffer holds %u)", n_cand, cand_cap);
            }
            return;
        }
        stats[0] += n_cand;
        if (n_cand == 0) return;
        const uint32_t n = (uint32_t)n_cand;
        const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)t->n_cu * 8, (n + 15) / 16));
        hipLaunchKernelGGL((assign_multi_rescore_kernel<NCH>), dim3(blocks), dim3(256), 0, s, qf, t->table, d_cand, n, m,
                           __builtin_inff(), 0u, d_slot);
        HIP_CHECK(hipGetLastError());
    }

    // qf / qm / qx / q_tomb / q_local0 / n_s describe the strip -> idx / dist of its n_s queries on the host
    template <int NCH>
    void strip(uint64_t* idx, float* dist) {
        const size_t el = (size_t)n_s * m;
        HIP_CHECK(hipMemsetAsync(d_slot, 0xFF, el * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_gslot, SMY_ORD_NINF, el, s));
        const uint32_t n_rt = (n_s + AMU_TILE - 1) / AMU_TILE;
        tiles<NCH, false>(0, n_rt, 0, sample, (n_cb + sample - 1) / sample);
        uint32_t piece = std::max(1u, std::min(n_rt, cand_cap / (AMU_TILE * 16u * m)));
        for (uint32_t br = 0; br < n_rt;) {
            const uint32_t end = std::min(n_rt, br + piece);
            const uint64_t before = stats[0];
            bool overflowed = false;
            rect<NCH>(br, end, 0, n_cb, &overflowed);
            // the next piece: half the buffer at the rate this one saw
            const uint64_t per_tile = (stats[0] - before) / (end - br) + 1;
            piece = overflowed ? std::max(1u, piece / 2) : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_rt, cand_cap / (2 * per_tile)));
            br = end;
        }
        const IdMap map{t->base, t->cyc_block, t->cyc_n, t->cyc_rank};
        hipLaunchKernelGGL(search_many_finalize_kernel, dim3((n_s + 255) / 256), dim3(256), 0, s, d_slot, q_tomb, q_local0, n_s, m,
                           self_drop ? 1u : 0u, map, d_idx, d_dist, d_hits);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(idx, d_idx, (size_t)n_s * k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(dist, d_dist, (size_t)n_s * k * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));   // the strip's buffers are the next strip's
    }

    void strip(uint64_t* idx, float* dist) {
        switch (t->dim / 64) {
            case 2: strip<2>(idx, dist); break;
            case 4: strip<4>(idx, dist); break;
            case 8: strip<8>(idx, dist); break;
            case 12: strip<12>(idx, dist); break;
            case 16: strip<16>(idx, dist); break;
        }
    }

    // nq queries on the host -> idx / dist [nq][k]
    void run_queries(const float* q, uint32_t nq, uint64_t* idx, float* dist) {
        d_qf = (float*)scratch.get((size_t)strip_rows * t->dim * sizeof(float));
        d_qm = (uint16_t*)scratch.get((size_t)strip_rows * t->dim * sizeof(uint16_t));
        d_qx = (float*)scratch.get((size_t)strip_rows * sizeof(float));
        qf = d_qf; qm = d_qm; qx = d_qx; q_tomb = nullptr; q_local0 = 0;
        for (uint32_t q0 = 0; q0 < nq; q0 += strip_rows) {
            n_s = std::min(strip_rows, nq - q0);
            HIP_CHECK(hipMemcpyAsync(d_qf, q + (size_t)q0 * t->dim, (size_t)n_s * t->dim * sizeof(float), hipMemcpyHostToDevice, s));
            mirror_rows(t, s, d_qf, 0, n_s, d_qm, d_qx);
            strip(idx + (size_t)q0 * k, dist + (size_t)q0 * k);
        }
        finish();
    }

    // the table's local rows first .. first + n - 1 as the queries, read where they lie
    void run_rows(uint32_t first, uint32_t n, uint64_t* idx, float* dist) {
        q_tomb = tomb;
        for (uint32_t q0 = 0; q0 < n; q0 += strip_rows) {
            n_s = std::min(strip_rows, n - q0);
            q_local0 = first + q0;
            qf = t->table + (size_t)q_local0 * t->dim;
            qm = mirror + (size_t)q_local0 * t->dim;
            qx = xx + q_local0;
            strip(idx + (size_t)q0 * k, dist + (size_t)q0 * k);
        }
        finish();
    }

    void finish() {
        unsigned long long hits = 0;
        HIP_CHECK(hipMemcpyAsync(&hits, d_hits, sizeof hits, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        stats[1] = hits;
        for (int i = 0; i < 4; ++i) t->search_many_stats[i] = stats[i];
    }

    // t->mu held, device selected, arguments checked, the table not empty; nq = the queries of the call
    void setup(mi_knn* table, uint32_t nq, uint32_t n_keep, bool drop) {
        t = table;
        k = n_keep;
        self_drop = drop;
        m = k + (drop ? 1u : 0u);
        s = knn_own_stream(t);
        // behind every write and search enqueued before this call, on whichever stream
        t->writes.begin(s);
        t->reads.begin(s);
        n_cols = (uint32_t)t->rows;
        n_cb = (n_cols + AMU_TILE - 1) / AMU_TILE;
        // the join's bound, unchanged (join_kernels.h): both operands are rounded to bf16
        const float eps2 = 0x1p-7f + 0x1p-16f + 4.1f * (float)(t->dim + 8) * 0x1p-24f + 2e-6f;
        thr = 2.0f * eps2;
        cand_cap = std::max<uint32_t>(AMU_CAP_MIN, t->join_cap);
        tomb = t->dead.empty() ? nullptr : t->d_tomb;
        // the threshold pass visits every sample-th column tile ("many_sample"; by default all of them: DESIGN.md 5.18)
        sample = t->many_sample > 0 ? (uint32_t)t->many_sample : 1u;
        sample = std::max(1u, std::min(sample, n_cb));
        // the mirror: the table's own when "prefilter" = 1 keeps one (caught up here as a search would), else one for this call
        uint16_t* mr = nullptr;
        float* x = nullptr;
        uint64_t from = 0;
        if (t->prefilter == 1) {
            t->mirror_rows = std::min(t->mirror_rows, t->rows);
            grow_keep(t, (void**)&t->d_mirror, &t->mirror_cap, (size_t)t->cap * t->dim, sizeof(uint16_t), (size_t)t->mirror_rows * t->dim);
            grow_keep(t, (void**)&t->d_xx, &t->xx_cap, (size_t)t->cap, sizeof(float), (size_t)t->mirror_rows);
            mr = t->d_mirror; x = t->d_xx; from = t->mirror_rows;
        } else {
            mr = (uint16_t*)scratch.get((size_t)t->rows * t->dim * sizeof(uint16_t));
            x = (float*)scratch.get((size_t)t->rows * sizeof(float));
        }
        if (from < t->rows) {
            mirror_rows(t, s, t->table, from, t->rows, mr, x);
            if (t->prefilter == 1) t->mirror_rows = t->rows;
        }
        mirror = mr; xx = x;
        strip_rows = (uint32_t)std::min<uint64_t>((uint64_t)STRIP_TILES * AMU_TILE, nq);
        const size_t strip_el = (size_t)strip_rows * m;
        d_cand = (uint2*)scratch.get((size_t)cand_cap * sizeof(uint2));
        d_count = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
        d_hits = d_count + 1;
        HIP_CHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), s));
        d_slot = (unsigned long long*)scratch.get(strip_el * sizeof(unsigned long long));
        d_gslot = (int*)scratch.get(strip_el * sizeof(int));
        d_idx = (uint64_t*)scratch.get((size_t)strip_rows * k * sizeof(uint64_t));
        d_dist = (float*)scratch.get((size_t)strip_rows * k * sizeof(float));
    }
};

// whatever happens, the handle's stream is idle and its order words say so when the call leaves
struct Settle {
    mi_knn* t; hipStream_t s;
    ~Settle() { (void)hipStreamSynchronize(s); t->reads.pending = false; }
};

void check_table(const mi_knn* t) {
    if (t->dim % 128 != 0 || (t->dim / 64 != 2 && t->dim / 64 != 4 && t->dim / 64 != 8 && t->dim / 64 != 12 && t->dim / 64 != 16))
        fail(MI_ERR_UNSUPPORTED, "dim %u: the bf16 mirror is built for dim in {128, 256, 512, 768, 1024}", t->dim);
    // (a shard never grows beyond this: the candidate record is a pair of uint32)
    if (t->rows > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "a shard holds at most 2^32-1 rows");
}

void check_args(const mi_knn* t, const float* q, uint32_t nq, uint32_t k, const uint64_t* idx, const float* dist) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (!q) fail(MI_ERR_INVALID, "q is null");
    if (!idx || !dist) fail(MI_ERR_INVALID, "idx / dist is null");
    if (nq == 0) fail(MI_ERR_INVALID, "nq must be >= 1");
    if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
    if (k > MAX_K) fail(MI_ERR_UNSUPPORTED, "at most %u neighbours per query (got %u)", MAX_K, k);
    check_table(t);
}

void pad(uint64_t* idx, float* dist, size_t n) {
    std::fill(idx, idx + n, MI_KNN_NO_ID);
    std::fill(dist, dist + n, INFINITY);
}

// the shard's answer, [nq][k]
void search_many_local(mi_knn* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->search_many_stats) v = 0;
    if (t->rows == 0) {
        pad(idx, dist, (size_t)nq * k);
        return;
    }
    DeviceGuard g(t->device);
    SearchMany a;
    a.setup(t, nq, k, false);
    Settle settle{t, a.s};
    a.run_queries(q, nq, idx, dist);
}

}  // namespace

extern "C" {

int mi_knn_search_many(mi_knn* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] {
        check_args(t, q, nq, k, idx, dist);
        search_many_local(t, q, nq, k, idx, dist);
    });
}

int mi_knn_search_many_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->search_many_stats[i];
    });
}

int mi_knn_neighbors(mi_knn* t, uint64_t first, uint64_t n, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
        if (k > MAX_K - 1) fail(MI_ERR_UNSUPPORTED, "at most %u neighbours per row (got %u)", MAX_K - 1, k);
        if (n != 0 && (!idx || !dist)) fail(MI_ERR_INVALID, "idx / dist is null");
        check_table(t);
        std::lock_guard<std::mutex> l(t->mu);
        if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "a shard of a sharded table holds no contiguous ids: use mi_knn_sharded_search_many");
        if (first < t->base || first - t->base > t->rows || n > t->rows - (first - t->base))
            fail(MI_ERR_INVALID, "rows [%llu,%llu) are not rows of this table (base %llu, %llu rows)", (unsigned long long)first,
                 (unsigned long long)(first + n), (unsigned long long)t->base, (unsigned long long)t->rows);
        for (uint64_t& v : t->search_many_stats) v = 0;
        if (n == 0) return;
        DeviceGuard g(t->device);
        SearchMany a;
        a.setup(t, (uint32_t)n, k, true);
        Settle settle{t, a.s};
        a.run_rows((uint32_t)(first - t->base), (uint32_t)n, idx, dist);
    });
}

int mi_knn_sharded_search_many(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (t->shard.empty()) fail(MI_ERR_INVALID, "a table without shards");
        check_args(t->shard[0], q, nq, k, idx, dist);
        std::lock_guard<std::mutex> l(t->mu);
        sharded_deliver_all(t);
        // every shard on its own stream, driven by a host thread of its own (a shard's search reads its candidate counts
        // back between launches); the lists carry global ids
        const uint32_t n = t->n();
        const size_t el = (size_t)nq * k;
        std::vector<uint64_t> all_idx(el * n);
        std::vector<float> all_dist(el * n);
        std::vector<int> codes(n, MI_OK);
        std::vector<std::string> msgs(n);
        std::vector<std::thread> threads;
        for (uint32_t si = 0; si < n; ++si) {
            threads.emplace_back([&, si] {
                try {
                    search_many_local(t->shard[si], q, nq, k, all_idx.data() + el * si, all_dist.data() + el * si);
                } catch (const Error& e) {
                    codes[si] = e.code; msgs[si] = e.what();
                } catch (const std::exception& e) {
                    codes[si] = MI_ERR_INVALID; msgs[si] = e.what();
                }
            });
        }
        for (std::thread& th : threads) th.join();
        for (uint32_t si = 0; si < n; ++si)
            if (codes[si] != MI_OK) fail(codes[si], "shard %u: %s", si, msgs[si].c_str());
        // mi_knn_merge's ordering, query by query
        std::vector<uint64_t> li((size_t)n * k);
        std::vector<float> ld((size_t)n * k);
        for (uint32_t u = 0; u < nq; ++u) {
            for (uint32_t si = 0; si < n; ++si) {
                std::memcpy(li.data() + (size_t)si * k, all_idx.data() + el * si + (size_t)u * k, k * sizeof(uint64_t));
                std::memcpy(ld.data() + (size_t)si * k, all_dist.data() + el * si + (size_t)u * k, k * sizeof(float));
            }
            merge_lists(li.data(), ld.data(), n, k, idx + (size_t)u * k, dist + (size_t)u * k);
        }
    });
}

}  // extern "C"
