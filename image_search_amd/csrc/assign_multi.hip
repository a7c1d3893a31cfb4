// assign_multi.hip — host side of mi_knn_assign_multi (every row labelled by up to m of C vectors, within max_dist) and of
// mi_knn_sharded_assign_multi.  The kernels and the superset argument: assign_multi_kernels.h.
//
// The rows are walked in strips of row tiles.  A strip owns the only per-row state of stage 2, its rows' m slots, so the
// device workspace beyond the rows' mirror is: the vectors (fp32 + bf16 mirror + norms), the candidate buffer ("join_cap"
// pairs of 8 bytes) and, for at most STRIP_MAX x 128 rows, the slots (8 m bytes per row) and the unpacked labels / dist
// (8 m bytes per row) — independent of the table's size.  A strip's results are copied out before the next strip starts.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "handles.h"
#include "assign_multi_kernels.h"

using namespace mi;
using namespace mi_assign_multi::mi;

namespace {

constexpr uint32_t ASSIGN_MAX_C = 65536;
constexpr uint32_t STRIP_MAX = 2048;   // row tiles of a strip

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

// the table's own mirror grows with its capacity, keeping the rows mirrored so far (as join.hip)
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

// One call's state: the rows' mirror, the vectors, one strip's slots and results on the device.
struct AssignMulti {
    mi_knn* t = nullptr;
    hipStream_t s = nullptr;
    Scratch scratch;
    uint32_t n_rows = 0, C = 0, m = 0, n_cb = 0, cand_cap = 0, strip = 0;
    float thr = 0.0f, cdist = 0.0f, max_dist = 0.0f;
    const uint16_t* mirror = nullptr;
    const float* xx = nullptr;
    const uint64_t* tomb = nullptr;
    float* d_vec = nullptr;          // [C][dim] fp32
    uint16_t* d_vmirror = nullptr;
    float* d_vxx = nullptr;
    uint2* d_cand = nullptr;
    unsigned long long *d_count = nullptr, *d_hits = nullptr, *d_slot = nullptr;
    uint32_t* d_labels = nullptr;    // [strip rows][m]
    float* d_dist = nullptr;
    uint32_t row_base = 0;           // first row of the strip under way
    uint64_t stats[4] = {0, 0, 0, 0};

    template <int NCH>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        if (bc0 >= bc1 || br0 >= br1) return;
        static DevOnce once;
        allow_lds_once(once, assign_multi_tiles_kernel<NCH>, AMU_LDS);
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL((assign_multi_tiles_kernel<NCH>), dim3(br1 - br0), dim3(256), AMU_LDS, s, mirror, xx, tomb, n_rows,
                           d_vmirror, d_vxx, C, m, br0, bc0, bc1, thr, cdist, cand_cap, d_cand, d_count);
        HIP_CHECK(hipGetLastError());
        unsigned long long n_cand = 0;
        HIP_CHECK(hipMemcpyAsync(&n_cand, d_count, sizeof n_cand, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ++stats[2];
        stats[3] += (uint64_t)(br1 - br0) * (bc1 - bc0);
        if (n_cand > cand_cap) {   // nothing is dropped: the same ground again in two halves, rows first, then columns
            if (overflowed) *overflowed = true;
            if (br1 - br0 > 1) {
                const uint32_t mid = br0 + (br1 - br0) / 2;
                rect<NCH>(br0, mid, bc0, bc1, nullptr);
                rect<NCH>(mid, br1, bc0, bc1, nullptr);
            } else if (bc1 - bc0 > 1) {   // (the row tile's slots of stage 2 live in d_slot: they join the column pieces)
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
        hipLaunchKernelGGL((assign_multi_rescore_kernel<NCH>), dim3(blocks), dim3(256), 0, s, t->table, d_vec, d_cand, n, m, max_dist,
                           row_base, d_slot);
        HIP_CHECK(hipGetLastError());
    }

    // d_vec holds the vectors: -> labels / dist on the host, strip by strip
    template <int NCH>
    void run(uint32_t* labels, float* dist) {
        launch_mirror<NCH>(s, t->n_cu, d_vec, 0, C, d_vmirror, d_vxx);
        HIP_CHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), s));
        const uint32_t n_rb = (n_rows + AMU_TILE - 1) / AMU_TILE;
        for (uint32_t br = 0; br < n_rb;) {
            const uint32_t end = std::min(n_rb, br + strip);
            row_base = br * AMU_TILE;
            const uint32_t n_local = std::min<uint32_t>(n_rows, end * AMU_TILE) - row_base;
            const size_t el = (size_t)n_local * m;
            HIP_CHECK(hipMemsetAsync(d_slot, 0xFF, el * sizeof(unsigned long long), s));
            bool overflowed = false;
            rect<NCH>(br, end, 0, n_cb, &overflowed);
            hipLaunchKernelGGL(assign_multi_finalize_kernel, dim3((uint32_t)((el + 255) / 256)), dim3(256), 0, s, d_slot, tomb, row_base,
                               n_local, m, d_labels, dist ? d_dist : (float*)nullptr, d_hits);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(labels + (size_t)row_base * m, d_labels, el * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            if (dist) HIP_CHECK(hipMemcpyAsync(dist + (size_t)row_base * m, d_dist, el * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));   // the strip's buffers are the next strip's
            if (overflowed) strip = std::max(1u, strip / 2);
            br = end;
        }
        unsigned long long hits = 0;
        HIP_CHECK(hipMemcpyAsync(&hits, d_hits, sizeof hits, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        stats[1] = hits;
        for (int i = 0; i < 4; ++i) t->assign_multi_stats[i] = stats[i];
    }

    void run(uint32_t* labels, float* dist) {
        switch (t->dim / 64) {
            case 2: run<2>(labels, dist); break;
            case 4: run<4>(labels, dist); break;
            case 8: run<8>(labels, dist); break;
            case 12: run<12>(labels, dist); break;
            case 16: run<16>(labels, dist); break;
        }
    }

    // t->mu held, device selected, arguments checked, the table not empty
    void setup(mi_knn* table, uint32_t n_vec, uint32_t n_lab, float md) {
        t = table;
        C = n_vec;
        m = n_lab;
        max_dist = md;
        s = knn_own_stream(t);
        // behind every write and search enqueued before this call, on whichever stream
        t->writes.begin(s);
        t->reads.begin(s);
        n_rows = (uint32_t)t->rows;
        n_cb = (C + AMU_TILE - 1) / AMU_TILE;
        // the join's bound, unchanged (join_kernels.h): both operands are rounded to bf16
        const float eps2 = 0x1p-7f + 0x1p-16f + 4.1f * (float)(t->dim + 8) * 0x1p-24f + 2e-6f;
        thr = 2.0f * eps2;
        cdist = 1.0f - (max_dist + eps2);   // the join's c; -inf without a threshold
        cand_cap = std::max<uint32_t>(AMU_CAP_MIN, t->join_cap);
        tomb = t->dead.empty() ? nullptr : t->d_tomb;
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
            switch (t->dim / 64) {
#define MI_CASE(NCH) case NCH: launch_mirror<NCH>(s, t->n_cu, t->table, from, t->rows, mr, x); break;
                MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
            }
            if (t->prefilter == 1) t->mirror_rows = t->rows;
        }
        mirror = mr; xx = x;
        // strips of row tiles: as many as keep an ordinary corpus (the running threshold of m slots lets a few candidates per
        // label, row and column tile through) inside the buffer
        const uint32_t n_rb = (n_rows + AMU_TILE - 1) / AMU_TILE;
        strip = std::max<uint32_t>(1u, std::min<uint32_t>({STRIP_MAX, n_rb, cand_cap / (AMU_TILE * 4u * m * n_cb)}));
        const size_t strip_el = (size_t)std::min<uint64_t>((uint64_t)strip * AMU_TILE, n_rows) * m;
        d_vec = (float*)scratch.get((size_t)C * t->dim * sizeof(float));
        d_vmirror = (uint16_t*)scratch.get((size_t)C * t->dim * sizeof(uint16_t));
        d_vxx = (float*)scratch.get((size_t)C * sizeof(float));
        d_cand = (uint2*)scratch.get((size_t)cand_cap * sizeof(uint2));
        d_count = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
        d_hits = d_count + 1;
        d_slot = (unsigned long long*)scratch.get(strip_el * sizeof(unsigned long long));
        d_labels = (uint32_t*)scratch.get(strip_el * sizeof(uint32_t));
        d_dist = (float*)scratch.get(strip_el * sizeof(float));
    }
};

// whatever happens, the handle's stream is idle and its order words say so when the call leaves
struct Settle {
    mi_knn* t; hipStream_t s;
    ~Settle() { (void)hipStreamSynchronize(s); t->reads.pending = false; }
};

void check_args(const mi_knn* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, const uint32_t* labels) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (!vectors) fail(MI_ERR_INVALID, "vectors is null");
    if (!labels) fail(MI_ERR_INVALID, "labels is null");
    if (C == 0) fail(MI_ERR_INVALID, "C must be >= 1");
    if (m == 0) fail(MI_ERR_INVALID, "m must be >= 1");
    if (!(max_dist >= 0.0f)) fail(MI_ERR_INVALID, "max_dist must be >= 0 (+inf: no threshold), not NaN");
    if (C > ASSIGN_MAX_C) fail(MI_ERR_UNSUPPORTED, "at most %u vectors (got %u)", ASSIGN_MAX_C, C);
    if (m > (uint32_t)AMU_MAX_M) fail(MI_ERR_UNSUPPORTED, "at most %d labels per row (got %u)", AMU_MAX_M, m);
    if (t->dim % 128 != 0 || (t->dim / 64 != 2 && t->dim / 64 != 4 && t->dim / 64 != 8 && t->dim / 64 != 12 && t->dim / 64 != 16))
        fail(MI_ERR_UNSUPPORTED, "dim %u: the assign's bf16 mirror is built for dim in {128, 256, 512, 768, 1024}", t->dim);
}

// labels / dist of the shard's local rows, [rows][m]
void assign_multi_local(mi_knn* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, uint32_t* labels, float* dist) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->assign_multi_stats) v = 0;
    if (t->rows == 0) return;
    DeviceGuard g(t->device);
    AssignMulti a;
    a.setup(t, C, m, max_dist);
    Settle settle{t, a.s};
    HIP_CHECK(hipMemcpyAsync(a.d_vec, vectors, (size_t)C * t->dim * sizeof(float), hipMemcpyHostToDevice, a.s));
    a.run(labels, dist);
}

}  // namespace

extern "C" {

int mi_knn_assign_multi(mi_knn* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, uint32_t* labels, float* dist) {
    return guarded([&] {
        check_args(t, vectors, C, m, max_dist, labels);
        assign_multi_local(t, vectors, C, m, max_dist, labels, dist);
    });
}

int mi_knn_assign_multi_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->assign_multi_stats[i];
    });
}

int mi_knn_sharded_assign_multi(mi_knn_sharded* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, uint32_t* labels,
                                float* dist) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (t->shard.empty()) fail(MI_ERR_INVALID, "a table without shards");
        check_args(t->shard[0], vectors, C, m, max_dist, labels);
        std::lock_guard<std::mutex> l(t->mu);
        sharded_deliver_all(t);
        // every shard on its own stream, driven by a host thread of its own (a shard's assign reads its candidate counts
        // back between launches); results land at the rows' global ids
        const uint32_t n = t->n();
        std::vector<int> codes(n, MI_OK);
        std::vector<std::string> msgs(n);
        std::vector<std::thread> threads;
        for (uint32_t si = 0; si < n; ++si) {
            threads.emplace_back([&, si] {
                try {
                    mi_knn* sh = t->shard[si];
                    const uint64_t rows = sh->rows;
                    std::vector<uint32_t> lab(rows * m);
                    std::vector<float> dd(dist ? rows * m : 0);
                    assign_multi_local(sh, vectors, C, m, max_dist, lab.data(), dist ? dd.data() : nullptr);
                    const IdMap map{sh->base, sh->cyc_block, sh->cyc_n, sh->cyc_rank};
                    for (uint64_t r = 0; r < rows; ++r) {
                        const uint64_t id = id_of_local(map, r);
                        std::memcpy(labels + id * m, lab.data() + r * m, m * sizeof(uint32_t));
                        if (dist) std::memcpy(dist + id * m, dd.data() + r * m, m * sizeof(float));
                    }
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
    });
}

}  // extern "C"
