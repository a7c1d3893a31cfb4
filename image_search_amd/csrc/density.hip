// density.hip — host side of mi_knn_density, mi_knn_dbscan, mi_knn_dbscan_stats and mi_index_themes.  The kernels, the
// exactness of the tile skip and the disjoint-set forest: density_kernels.h; the host-only rules: density_host.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <mutex>
#include <vector>

#include "common.h"
#include "density_host.h"
#include "density_kernels.h"
#include "handles.h"
#include "two_stage.h"

using namespace mi;

namespace {

struct Density {
    mi_knn* t;
    hipStream_t s;
    const uint16_t* mirror;
    const float* xx;
    const uint64_t* tomb;
    uint32_t n_rows, n_blocks, min_pts;
    float max_dist, c;
    uint32_t cand_cap;
    uint2* d_cand;
    unsigned long long* d_words;   // DW_* of density_kernels.h
    uint32_t *d_deg, *d_parent;
    unsigned long long* d_bkey;
    uint8_t* d_act;
    DensityBlocks blocks;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // One pass's stages for rect_stages (two_stage.h), the join's rectangle: tiles on or above the diagonal.  rect_stages
    // hands a candidate buffer to stage 2 only when the launch that filled it fitted, and redoes the ground of one that did
    // not in halves without consuming anything: every pair of W reaches stage 2 exactly once, also across overflow halvings.
    // Degrees (adds) rely on that; unions and minima would not mind a repeat.  The tile counts follow the same rule: only
    // the launches whose candidates were consumed are counted, so visited + skipped is the triangle.
    template <int NCH, int PASS>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) -> unsigned long long {
            c0 = std::max(c0, r0);
            if (c0 >= c1) return 0;
            uint64_t visited = 0, skipped = 0;
            if (PASS == 2) {
                blocks.count(r0, r1, c0, c1, &visited, &skipped);
                if (visited == 0) { stats[5] += skipped; return 0; }   // every workgroup would leave at once
            } else {
                for (uint32_t bi = r0; bi < r1; ++bi) visited += c1 - std::max(c0, bi);
            }
            HIP_CHECK(hipMemsetAsync(d_words + DW_CAND, 0, sizeof(unsigned long long), s));
            if (PASS == 1) {
                static DevOnce once;
                allow_lds_once(once, join_tiles_kernel<NCH>, JOIN_LDS);
                hipLaunchKernelGGL((join_tiles_kernel<NCH>), dim3(c1 - c0, r1 - r0), dim3(256), JOIN_LDS, s, mirror, xx, tomb, n_rows, 0u,
                                   r0, c0, c, cand_cap, d_cand, d_words + DW_CAND);
            } else {
                static DevOnce once;
                allow_lds_once(once, density_tiles_kernel<NCH>, JOIN_LDS);
                hipLaunchKernelGGL((density_tiles_kernel<NCH>), dim3(c1 - c0, r1 - r0), dim3(256), JOIN_LDS, s, mirror, xx, tomb,
                                   (const uint8_t*)d_act, n_rows, r0, c0, c, cand_cap, d_cand, d_words + DW_CAND);
            }
            HIP_CHECK(hipGetLastError());
            ++stats[7];
            const unsigned long long n = read_count(d_words + DW_CAND, s);
            if (n <= cand_cap) {
                if (PASS == 1) stats[2] += visited;
                else { stats[4] += visited; stats[5] += skipped; }
            }
            return n;
        };
        auto stage2 = [&](uint32_t C) {
            if (PASS == 1) {
                stats[0] += C;
                hipLaunchKernelGGL((density_count_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, d_cand, C, max_dist,
                                   d_deg, d_words);
            } else {
                stats[3] += C;
                hipLaunchKernelGGL((density_link_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, d_cand, C, max_dist,
                                   min_pts, d_deg, d_parent, d_bkey, d_words);
            }
            HIP_CHECK(hipGetLastError());
        };
        rect_stages(br0, br1, bc0, bc1, cand_cap, overflowed, stage1, stage2);
    }

    // the join's strips (Join::run)
    template <int NCH, int PASS>
    void pass() {
        uint32_t strip = std::max<uint32_t>(1u, std::min<uint32_t>(256u, (1u << 18) / std::max(n_blocks, 1u)));
        for (uint32_t br = 0; br < n_blocks;) {
            const uint32_t end = std::min(n_blocks, br + strip);
            bool overflowed = false;
            rect<NCH, PASS>(br, end, 0, n_blocks, &overflowed);
            if (overflowed) strip = std::max(1u, strip / 2);
            br = end;
        }
    }
};

struct DensityOut {
    std::vector<uint64_t> cluster, via;
    std::vector<float> via_dist;
    std::vector<uint32_t> counts;
    uint64_t summary[4] = {0, 0, 0, 0};
};

// min_pts == 0: the degrees only (mi_knn_density).  want_*: which optional arrays to fetch.  Everything lands in `out`; the
// caller's arrays are written by the caller once this has returned.
void density_run(mi_knn* t, float max_dist, uint32_t min_pts, bool want_via, bool want_via_dist, bool want_counts, DensityOut* out) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->dbscan_stats) v = 0;
    check_mirror_dim(t->dim, "the density pass's");
    const uint64_t rows = t->rows;
    if (rows >= (1ull << 32)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)rows);
    if (rows == 0) return;
    Scratch scratch;
    TableCall call(t);
    hipStream_t s = call.s;
    Density d;
    d.t = t; d.s = s;
    d.n_rows = (uint32_t)rows;
    d.n_blocks = (uint32_t)((rows + TILE - 1) / TILE);
    d.min_pts = min_pts;
    d.max_dist = max_dist;
    d.c = 1.0f - (max_dist + eps2(t->dim));
    d.cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
    d.tomb = t->dead.empty() ? nullptr : t->d_tomb;
    d.mirror = nullptr; d.xx = nullptr;
    d.d_deg = (uint32_t*)scratch.get(rows * sizeof(uint32_t));
    d.d_words = (unsigned long long*)scratch.get(DW_WORDS * sizeof(unsigned long long));
    HIP_CHECK(hipMemsetAsync(d.d_deg, 0, rows * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(d.d_words, 0, DW_WORDS * sizeof(unsigned long long), s));
    const bool pairs_possible = rows >= 2;
    if (pairs_possible) {
        const TableMirror tm = table_mirror(t, s, scratch);
        d.mirror = tm.mirror; d.xx = tm.xx; d.tomb = tm.tomb;
        d.d_cand = (uint2*)scratch.get((size_t)d.cand_cap * sizeof(uint2));
        dispatch_nch(t->dim, [&](auto nch) { d.template pass<decltype(nch)::value, 1>(); });
    }

    unsigned long long words[DW_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (min_pts == 0) {
        out->counts.resize(rows);
        HIP_CHECK(hipMemcpyAsync(out->counts.data(), d.d_deg, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(words, d.d_words, sizeof words, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        d.stats[1] = words[DW_WITHIN];
        for (int i = 0; i < 8; ++i) t->dbscan_stats[i] = d.stats[i];
        return;
    }

    d.d_parent = (uint32_t*)scratch.get(rows * sizeof(uint32_t));
    d.d_bkey = (unsigned long long*)scratch.get(rows * sizeof(unsigned long long));
    d.d_act = (uint8_t*)scratch.get(d.n_blocks);
    hipLaunchKernelGGL(density_blocks_kernel, dim3(d.n_blocks), dim3(TILE), 0, s, d.d_deg, d.tomb, d.n_rows, min_pts, d.d_parent, d.d_bkey,
                       d.d_act);
    HIP_CHECK(hipGetLastError());
    if (pairs_possible) {
        // the activity bytes, read back once: the host counts from them what the tiles of pass 2 do
        d.blocks.act.resize(d.n_blocks);
        HIP_CHECK(hipMemcpyAsync(d.blocks.act.data(), d.d_act, d.n_blocks, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        d.blocks.index();
        dispatch_nch(t->dim, [&](auto nch) { d.template pass<decltype(nch)::value, 2>(); });
    }

    uint64_t* d_cluster = (uint64_t*)scratch.get(rows * sizeof(uint64_t));
    uint64_t* d_via = want_via ? (uint64_t*)scratch.get(rows * sizeof(uint64_t)) : nullptr;
    float* d_via_dist = want_via_dist ? (float*)scratch.get(rows * sizeof(float)) : nullptr;
    const IdMap map = knn_id_map(t);
    hipLaunchKernelGGL(density_finish_kernel, dim3((d.n_rows + 255) / 256), dim3(256), 0, s, d.d_deg, d.d_parent, d.d_bkey, d.tomb, d.n_rows,
                       min_pts, map, d_cluster, d_via, d_via_dist, d.d_words);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(words, d.d_words, sizeof words, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (words[DW_ERROR] != 0)
        fail(MI_ERR_HIP, "internal error: a step cap of the disjoint-set forest expired (%llu times); nothing was written",
             (unsigned long long)words[DW_ERROR]);
    out->cluster.resize(rows);
    HIP_CHECK(hipMemcpyAsync(out->cluster.data(), d_cluster, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (want_via) {
        out->via.resize(rows);
        HIP_CHECK(hipMemcpyAsync(out->via.data(), d_via, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    }
    if (want_via_dist) {
        out->via_dist.resize(rows);
        HIP_CHECK(hipMemcpyAsync(out->via_dist.data(), d_via_dist, rows * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if (want_counts) {
        // (a deleted row is in no pair: its degree is the 0 the contract names)
        out->counts.resize(rows);
        HIP_CHECK(hipMemcpyAsync(out->counts.data(), d.d_deg, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) out->summary[i] = words[DW_SUMMARY + i];
    d.stats[1] = words[DW_WITHIN];
    d.stats[6] = words[DW_MERGED];
    for (int i = 0; i < 8; ++i) t->dbscan_stats[i] = d.stats[i];
}

template <class T>
void copy_out(const std::vector<T>& v, T* p) {
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
}

}  // namespace

extern "C" {

int mi_knn_density(mi_knn* t, float max_dist, uint32_t* counts) {
    return guarded([&] {
        const char* why = "";
        const int bad = density_check_args(t, max_dist, counts, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        DensityOut out;
        density_run(t, max_dist, 0, false, false, true, &out);
        copy_out(out.counts, counts);
    });
}

int mi_knn_dbscan(mi_knn* t, float max_dist, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist, uint32_t* counts,
                  uint64_t summary[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = dbscan_check_args(t, max_dist, min_pts, cluster, summary, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        DensityOut out;
        density_run(t, max_dist, min_pts, via != nullptr, via_dist != nullptr, counts != nullptr, &out);
        copy_out(out.cluster, cluster);
        copy_out(out.via, via);
        copy_out(out.via_dist, via_dist);
        copy_out(out.counts, counts);
        for (int i = 0; i < 4; ++i) summary[i] = out.summary[i];
    });
}

int mi_knn_dbscan_stats(mi_knn* t, uint64_t out[8]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 8; ++i) out[i] = t->dbscan_stats[i];
    });
}

int mi_index_themes(mi_index* ix, float max_dist, uint32_t min_pts, uint64_t* ids, uint64_t cap_ids, uint64_t* group_start,
                    uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups, uint64_t* n_noise) {
    return guarded([&] {
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        if (!(max_dist >= 0.0f)) fail(MI_ERR_INVALID, "max_dist must be a number >= 0 (got %g)", (double)max_dist);
        if (min_pts == 0) fail(MI_ERR_INVALID, "min_pts must be >= 1 (it counts the row itself)");
        if (!n_ids || !n_groups || !n_noise) fail(MI_ERR_INVALID, "n_ids, n_groups or n_noise is null");
        if ((cap_ids && !ids) || (cap_groups && !group_start)) fail(MI_ERR_INVALID, "an output array is null with a cap > 0");
        mi_knn* t = mi_index_table(ix);
        if (!t) fail(MI_ERR_INVALID, "the index has no table");
        // (a removed path's rows are deleted rows of the table: they are in no cluster and are not noise)
        DensityOut out;
        density_run(t, max_dist, min_pts, false, false, false, &out);
        IdMap map;
        {
            std::lock_guard<std::mutex> l(t->mu);
            map = knn_id_map(t);
        }
        std::vector<uint64_t> row_ids(out.cluster.size());
        for (size_t r = 0; r < row_ids.size(); ++r) row_ids[r] = id_of_local(map, r);
        std::vector<uint64_t> gids, starts;
        density_lists(row_ids.data(), out.cluster.data(), row_ids.size(), &gids, &starts);
        *n_ids = gids.size();
        *n_groups = starts.size() - 1;
        *n_noise = out.summary[3];
        if (ids) std::copy(gids.begin(), gids.begin() + (size_t)std::min<uint64_t>(cap_ids, gids.size()), ids);
        if (group_start) std::copy(starts.begin(), starts.begin() + (size_t)std::min<uint64_t>(cap_groups, starts.size()), group_start);
    });
}

}  // extern "C"
