// density_levels.hip — host side of mi_knn_density_levels, mi_knn_dbscan_levels and mi_dbscan_levels_tree.  The kernels and
// why one pair of tile passes serves every level: density_levels_kernels.h; the host-only rules: density_levels_host.h.  Stage 1
// of both passes, with its overflow scheme and tile counts, is density_call.h's under the top level's bound; the strips are
// tile_strips (join_between_host.h).
#include <algorithm>
#include <cstring>

#include <mutex>
#include <vector>

#include "common.h"
#include "density_call.h"
#include "density_host.h"
#include "density_levels_host.h"
#include "density_levels_kernels.h"
#include "handles.h"
#include "two_stage.h"

using namespace mi;

namespace {

struct LevelsCall {
    mi_knn* t;
    hipStream_t s;
    uint32_t n_rows, n_blocks;
    DensityLevels lv;
    unsigned long long* d_words;   // DWL_* of density_levels_kernels.h
    uint32_t *d_deg, *d_parent;    // [lv.n][n_rows]
    unsigned long long* d_bkey;    // [lv.n][n_rows]
    uint8_t *d_core_from, *d_act;
    DensityBlocks blocks;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DensityStage1<true> st1;       // stage 1 of both passes under the top level's bound (density_call.h)

    // Density::pass with this unit's second stages: every pair of the top level's W reaches stage 2 exactly once, also
    // across overflow halvings (the bins are adds)
    template <int NCH, int PASS>
    void pass() {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) { return st1.template stage1<NCH, PASS>(r0, r1, c0, c1); };
        auto stage2 = [&](uint32_t C) {
            if (PASS == 1) {
                stats[0] += C;
                hipLaunchKernelGGL((density_count_levels_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, st1.d_cand, C,
                                   lv, n_rows, d_deg, d_words);
            } else {
                stats[3] += C;
                hipLaunchKernelGGL((density_link_levels_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, st1.d_cand, C, lv,
                                   n_rows, (const uint8_t*)d_core_from, d_parent, d_bkey, d_words);
            }
            HIP_CHECK(hipGetLastError());
        };
        tile_strips(0, n_blocks, 0, n_blocks,
                    [&](uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
                        rect_stages(br0, br1, bc0, bc1, st1.cand_cap, overflowed, stage1, stage2);
                    },
                    [] { return false; });
    }
};

struct LevelsOut {   // every array [n_levels][rows]
    std::vector<uint64_t> cluster, via;
    std::vector<float> via_dist;
    std::vector<uint32_t> counts;
    uint64_t summary[MI_KNN_LEVELS_MAX][4] = {};
};

// min_pts == 0: the degrees only (mi_knn_density_levels).  Everything lands in `out`; the caller's arrays are written by the
// caller once this has returned.
void levels_run(mi_knn* t, const DensityLevels& lv, uint32_t min_pts, bool want_via, bool want_via_dist, bool want_counts, LevelsOut* out) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->dbscan_stats) v = 0;
    check_mirror_dim(t->dim, "the density pass's");
    const uint64_t rows = t->rows;
    if (rows >= (1ull << 32)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)rows);
    if (rows == 0) return;
    const uint64_t cells = rows * lv.n;
    Scratch scratch;
    TableCall call(t);
    hipStream_t s = call.s;
    LevelsCall d;
    d.t = t; d.s = s;
    d.n_rows = (uint32_t)rows;
    d.n_blocks = (uint32_t)((rows + TILE - 1) / TILE);
    d.lv = lv;
    const uint64_t* tomb = t->dead.empty() ? nullptr : t->d_tomb;
    d.d_deg = (uint32_t*)scratch.get(cells * sizeof(uint32_t));
    d.d_words = (unsigned long long*)scratch.get(DWL_WORDS * sizeof(unsigned long long));
    HIP_CHECK(hipMemsetAsync(d.d_deg, 0, cells * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(d.d_words, 0, DWL_WORDS * sizeof(unsigned long long), s));
    const bool pairs_possible = rows >= 2;
    if (pairs_possible) {
        const TableMirror tm = table_mirror(t, s, scratch);
        DensityStage1<true>& st = d.st1;
        st.s = s;
        st.a = st.b = DensitySide{tm.mirror, tm.xx, tm.tomb, d.n_rows, nullptr};
        st.blocks = &d.blocks; st.cross = nullptr;
        st.c = 1.0f - (lv.d[lv.n - 1] + eps2(t->dim));   // the top level's bound
        st.cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
        st.d_cand = (uint2*)scratch.get((size_t)st.cand_cap * sizeof(uint2));
        st.d_count = d.d_words + DWL_CAND;
        st.stats = d.stats;
        dispatch_nch(t->dim, [&](auto nch) { d.template pass<decltype(nch)::value, 1>(); });
    }

    unsigned long long words[DWL_WORDS];
    auto finish_stats = [&] {
        for (uint32_t m = 0; m < lv.n; ++m) d.stats[1] += words[DWL_WITHIN + m];   // the top level's pairs: every bin
        d.stats[6] = words[DWL_MERGED];
        for (int i = 0; i < 8; ++i) t->dbscan_stats[i] = d.stats[i];
    };
    if (min_pts == 0) {
        hipLaunchKernelGGL(density_levels_blocks_kernel, dim3(d.n_blocks), dim3(TILE), 0, s, d.d_deg, tomb, d.n_rows, lv.n, 0u,
                           (uint32_t*)nullptr, (unsigned long long*)nullptr, (uint8_t*)nullptr, (uint8_t*)nullptr);
        HIP_CHECK(hipGetLastError());
        read_back(&out->counts, d.d_deg, cells, s);
        HIP_CHECK(hipMemcpyAsync(words, d.d_words, sizeof words, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        finish_stats();
        return;
    }

    d.d_parent = (uint32_t*)scratch.get(cells * sizeof(uint32_t));
    d.d_bkey = (unsigned long long*)scratch.get(cells * sizeof(unsigned long long));
    d.d_core_from = (uint8_t*)scratch.get(rows);
    d.d_act = (uint8_t*)scratch.get(d.n_blocks);
    hipLaunchKernelGGL(density_levels_blocks_kernel, dim3(d.n_blocks), dim3(TILE), 0, s, d.d_deg, tomb, d.n_rows, lv.n, min_pts, d.d_parent,
                       d.d_bkey, d.d_core_from, d.d_act);
    HIP_CHECK(hipGetLastError());
    if (pairs_possible) {
        // the activity bytes, read back once: the host counts from them what the tiles of pass 2 do
        d.blocks.act.resize(d.n_blocks);
        HIP_CHECK(hipMemcpyAsync(d.blocks.act.data(), d.d_act, d.n_blocks, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        d.blocks.index();
        d.st1.a.act = d.st1.b.act = d.d_act;
        dispatch_nch(t->dim, [&](auto nch) { d.template pass<decltype(nch)::value, 2>(); });
    }

    uint64_t* d_cluster = (uint64_t*)scratch.get(cells * sizeof(uint64_t));
    uint64_t* d_via = want_via ? (uint64_t*)scratch.get(cells * sizeof(uint64_t)) : nullptr;
    float* d_via_dist = want_via_dist ? (float*)scratch.get(cells * sizeof(float)) : nullptr;
    const IdMap map = knn_id_map(t);
    hipLaunchKernelGGL(density_levels_finish_kernel, dim3((d.n_rows + 255) / 256, lv.n), dim3(256), 0, s, d.d_parent, d.d_bkey,
                       (const uint8_t*)d.d_core_from, tomb, d.n_rows, map, d_cluster, d_via, d_via_dist, d.d_words);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(words, d.d_words, sizeof words, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (words[DWL_ERROR] != 0)
        fail(MI_ERR_HIP, "internal error: a step cap of the disjoint-set forest expired (%llu times); nothing was written",
             (unsigned long long)words[DWL_ERROR]);
    read_back(&out->cluster, d_cluster, cells, s);
    if (want_via) read_back(&out->via, d_via, cells, s);
    if (want_via_dist) read_back(&out->via_dist, d_via_dist, cells, s);
    if (want_counts) read_back(&out->counts, d.d_deg, cells, s);
    HIP_CHECK(hipStreamSynchronize(s));
    for (uint32_t m = 0; m < lv.n; ++m)
        for (int i = 0; i < 4; ++i) out->summary[m][i] = words[DWL_SUMMARY + 4 * m + i];
    finish_stats();
}

}  // namespace

extern "C" {

int mi_knn_density_levels(mi_knn* t, const float* max_dists, uint32_t n_levels, uint32_t* counts) {
    return guarded([&] {
        const char* why = "";
        const int bad = density_levels_check_args(t, max_dists, n_levels, counts, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        LevelsOut out;
        levels_run(t, density_levels_make(max_dists, n_levels), 0, false, false, true, &out);
        copy_out(out.counts, counts);
    });
}

int mi_knn_dbscan_levels(mi_knn* t, const float* max_dists, uint32_t n_levels, uint32_t min_pts, uint64_t* cluster, uint64_t* via,
                         float* via_dist, uint32_t* counts, uint64_t* summary) {
    return guarded([&] {
        const char* why = "";
        const int bad = dbscan_levels_check_args(t, max_dists, n_levels, min_pts, cluster, summary, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        LevelsOut out;
        levels_run(t, density_levels_make(max_dists, n_levels), min_pts, via != nullptr, via_dist != nullptr, counts != nullptr, &out);
        copy_out(out.cluster, cluster);
        copy_out(out.via, via);
        copy_out(out.via_dist, via_dist);
        copy_out(out.counts, counts);
        for (uint32_t m = 0; m < n_levels; ++m)
            for (int i = 0; i < 4; ++i) summary[4 * m + i] = out.summary[m][i];
    });
}

int mi_dbscan_levels_tree(const uint64_t* cluster, const uint32_t* counts, uint64_t rows, uint32_t n_levels, uint32_t min_pts,
                          uint32_t* level, uint64_t* child, uint64_t* parent, uint64_t cap, uint64_t* n_edges) {
    return guarded([&] {
        if (!n_edges) fail(MI_ERR_INVALID, "n_edges is null");
        if (!cluster || !counts) fail(MI_ERR_INVALID, "cluster or counts is null");
        if (cap && (!level || !child || !parent)) fail(MI_ERR_INVALID, "an output array is null with a cap > 0");
        const char* why = "";
        std::vector<LevelEdge> edges;
        const int bad = dbscan_levels_tree(cluster, counts, rows, n_levels, min_pts, &edges, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        *n_edges = edges.size();
        const size_t n = (size_t)std::min<uint64_t>(cap, edges.size());
        for (size_t i = 0; i < n; ++i) {
            level[i] = edges[i].level;
            child[i] = edges[i].child;
            parent[i] = edges[i].parent;
        }
    });
}

}  // extern "C"
