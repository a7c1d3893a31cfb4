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
#include <vector>

#include "common.h"
#include "handles.h"
#include "assign_multi_kernels.h"
#include "sharded_call.h"
#include "two_stage.h"

using namespace mi;

namespace mi {

// a strip's slots -> labels / dist of its n_local rows, [n_local][m]; MI_KNN_NO_LABEL / +inf behind a row's last hit and for
// every entry of a deleted row.  dist may be null.  *hits += the (row, label) entries written (an integer count).
__global__ __launch_bounds__(256) void assign_multi_finalize_kernel(const unsigned long long* __restrict__ slot,
                                                                    const uint64_t* __restrict__ tomb, uint32_t row_base,
                                                                    uint32_t n_local, uint32_t m, uint32_t* __restrict__ labels,
                                                                    float* __restrict__ dist, unsigned long long* __restrict__ hits) {
    const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool is_hit = false;
    if (at < (uint64_t)n_local * m) {
        const uint32_t r = row_base + (uint32_t)(at / m);
        const bool dead = tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull);
        const unsigned long long key = slot[at];
        uint32_t lab = MI_KNN_NO_LABEL;
        float d = __uint_as_float(0x7F800000u);
        if (!dead && key != KEY_MAX) {
            lab = (uint32_t)key;
            d = u32_to_dist((uint32_t)(key >> 32));
            is_hit = true;
        }
        labels[at] = lab;
        if (dist) dist[at] = d;
    }
    const unsigned long long b = __ballot(is_hit);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(hits, (unsigned long long)__popcll(b));
}

}  // namespace mi

namespace {

constexpr uint32_t ASSIGN_MAX_C = 65536;
constexpr uint32_t STRIP_MAX = 2048;   // row tiles of a strip

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
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) {
            static DevOnce once;
            allow_lds_once(once, assign_multi_tiles_kernel<NCH>, AMU_LDS);
            HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL((assign_multi_tiles_kernel<NCH>), dim3(r1 - r0), dim3(256), AMU_LDS, s, mirror, xx, tomb, n_rows,
                               d_vmirror, d_vxx, C, m, r0, c0, c1, thr, cdist, cand_cap, d_cand, d_count);
            HIP_CHECK(hipGetLastError());
            ++stats[2];
            stats[3] += (uint64_t)(r1 - r0) * (c1 - c0);
            return read_count(d_count, s);
        };
        auto stage2 = [&](uint32_t n) {   // (the row tile's slots of stage 2 live in d_slot: they join the column pieces)
            stats[0] += n;
            hipLaunchKernelGGL((assign_multi_rescore_kernel<NCH>), dim3(group16_blocks(t, n)), dim3(256), 0, s, t->table, d_vec, d_cand,
                               n, m, max_dist, row_base, d_slot);
            HIP_CHECK(hipGetLastError());
        };
        rect_stages(br0, br1, bc0, bc1, cand_cap, overflowed, stage1, stage2);
    }

    // d_vec holds the vectors: -> labels / dist on the host, strip by strip
    template <int NCH>
    void run(uint32_t* labels, float* dist) {
        mirror_rows(t, s, d_vec, 0, C, d_vmirror, d_vxx);
        HIP_CHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), s));
        const uint32_t n_rb = (n_rows + TILE - 1) / TILE;
        for (uint32_t br = 0; br < n_rb;) {
            const uint32_t end = std::min(n_rb, br + strip);
            row_base = br * TILE;
            const uint32_t n_local = std::min<uint32_t>(n_rows, end * TILE) - row_base;
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
        dispatch_nch(t->dim, [&](auto nch) { run<decltype(nch)::value>(labels, dist); });
    }

    // inside the call's frame (declared after this object: the stream is idle before the scratch memory goes); arguments
    // checked, the table not empty
    void setup(const TableCall& call, uint32_t n_vec, uint32_t n_lab, float md) {
        t = call.t;
        C = n_vec;
        m = n_lab;
        max_dist = md;
        s = call.s;
        n_rows = (uint32_t)t->rows;
        n_cb = (C + TILE - 1) / TILE;
        const float e2 = eps2(t->dim);   // the join's bound, unchanged (join_kernels.h): both operands are rounded to bf16
        thr = 2.0f * e2;
        cdist = 1.0f - (max_dist + e2);   // the join's c; -inf without a threshold
        cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
        const TableMirror tm = table_mirror(t, s, scratch);
        mirror = tm.mirror; xx = tm.xx; tomb = tm.tomb;
        // strips of row tiles: as many as keep an ordinary corpus (the running threshold of m slots lets a few candidates per
        // label, row and column tile through) inside the buffer
        const uint32_t n_rb = (n_rows + TILE - 1) / TILE;
        strip = std::max<uint32_t>(1u, std::min<uint32_t>({STRIP_MAX, n_rb, cand_cap / (TILE * 4u * m * n_cb)}));
        const size_t strip_el = (size_t)std::min<uint64_t>((uint64_t)strip * TILE, n_rows) * m;
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

void check_args(const mi_knn* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, const uint32_t* labels) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (!vectors) fail(MI_ERR_INVALID, "vectors is null");
    if (!labels) fail(MI_ERR_INVALID, "labels is null");
    if (C == 0) fail(MI_ERR_INVALID, "C must be >= 1");
    if (m == 0) fail(MI_ERR_INVALID, "m must be >= 1");
    if (!(max_dist >= 0.0f)) fail(MI_ERR_INVALID, "max_dist must be >= 0 (+inf: no threshold), not NaN");
    if (C > ASSIGN_MAX_C) fail(MI_ERR_UNSUPPORTED, "at most %u vectors (got %u)", ASSIGN_MAX_C, C);
    if (m > (uint32_t)AMU_MAX_M) fail(MI_ERR_UNSUPPORTED, "at most %d labels per row (got %u)", AMU_MAX_M, m);
    check_mirror_dim(t->dim, "the assign's");
}

// labels / dist of the shard's local rows, [rows][m]
void assign_multi_local(mi_knn* t, const float* vectors, uint32_t C, uint32_t m, float max_dist, uint32_t* labels, float* dist) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->assign_multi_stats) v = 0;
    if (t->rows == 0) return;
    AssignMulti a;
    TableCall call(t);
    a.setup(call, C, m, max_dist);
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
        ShardedCall call(t);
        check_args(t->shard[0], vectors, C, m, max_dist, labels);
        // every shard on its own stream; results land at the rows' global ids
        call.for_each_shard([&](uint32_t, mi_knn* sh) {
            const uint64_t rows = sh->rows;
            std::vector<uint32_t> lab(rows * m);
            std::vector<float> dd(dist ? rows * m : 0);
            assign_multi_local(sh, vectors, C, m, max_dist, lab.data(), dist ? dd.data() : nullptr);
            const IdMap map = knn_id_map(sh);
            for (uint64_t r = 0; r < rows; ++r) {
                const uint64_t id = id_of_local(map, r);
                std::memcpy(labels + id * m, lab.data() + r * m, m * sizeof(uint32_t));
                if (dist) std::memcpy(dist + id * m, dd.data() + r * m, m * sizeof(float));
            }
        });
    });
}

}  // extern "C"
