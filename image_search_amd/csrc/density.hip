// density.hip — host side of mi_knn_density, mi_knn_dbscan, mi_knn_dbscan_stats and mi_index_themes, and of their windowed
// forms (mi_knn_density_window, mi_knn_dbscan_window, mi_index_events: the same passes with window.hip's stage 1, i.e. over
// W_win in place of W).  The kernels, the
// exactness of the tile skip and the disjoint-set forest: density_kernels.h; the host-only rules: density_host.h; stage 1 of
// the passes, shared with the levels and the sharded passes: density_call.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <mutex>
#include <vector>

#include "common.h"
#include "density_call.h"
#include "density_host.h"
#include "density_kernels.h"
#include "handles.h"
#include "two_stage.h"
#include "window_call.h"

using namespace mi;

namespace {

struct Density {
    mi_knn* t;
    hipStream_t s;
    uint32_t n_blocks, min_pts;
    float max_dist;
    unsigned long long* d_words;   // DW_* of density_kernels.h
    uint32_t *d_deg, *d_parent;
    unsigned long long* d_bkey;
    uint8_t* d_act;
    DensityBlocks blocks;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DensityStage1<true> st1;       // the table's mirror, the candidate buffer and stage 1 of both passes (density_call.h)
    WindowCall* win = nullptr;     // the windowed passes: stage 1 is window.hip's (it keeps the tile and launch counts)

    // one pass over the join's triangle in the join's strips: stage 1 is st1's, stage 2 this unit's
    template <int NCH, int PASS>
    void pass() {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) {
            return win ? window_stage1(*win, PASS, r0, r1, c0, c1) : st1.template stage1<NCH, PASS>(r0, r1, c0, c1);
        };
        auto stage2 = [&](uint32_t C) {
            if (PASS == 1) {
                stats[0] += C;
                hipLaunchKernelGGL((density_count_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, st1.d_cand, C,
                                   max_dist, d_deg, d_words);
            } else {
                stats[3] += C;
                hipLaunchKernelGGL((density_link_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, st1.d_cand, C, max_dist,
                                   min_pts, d_deg, d_parent, d_bkey, d_words);
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

struct DensityOut {
    std::vector<uint64_t> cluster, via;
    std::vector<float> via_dist;
    std::vector<uint32_t> counts;
    uint64_t summary[4] = {0, 0, 0, 0};
};

// min_pts == 0: the degrees only (mi_knn_density).  want_*: which optional arrays to fetch.  Everything lands in `out`; the
// caller's arrays are written by the caller once this has returned.  window (nullable): the passes run over W_win, the pairs
// whose stamps lie within *window of each other; the call's figures then go to t->window_stats and t->dbscan_stats stays as it is.
void density_run(mi_knn* t, float max_dist, uint32_t min_pts, bool want_via, bool want_via_dist, bool want_counts, DensityOut* out,
                 const uint64_t* window = nullptr) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : window ? t->window_stats : t->dbscan_stats) v = 0;
    check_mirror_dim(t->dim, "the density pass's");
    const uint64_t rows = t->rows;
    if (rows >= (1ull << 32)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)rows);
    if (rows == 0) return;
    Scratch scratch;
    TableCall call(t);
    hipStream_t s = call.s;
    Density d;
    d.t = t; d.s = s;
    d.n_blocks = (uint32_t)((rows + TILE - 1) / TILE);
    d.min_pts = min_pts;
    d.max_dist = max_dist;
    const uint32_t n_rows = (uint32_t)rows;
    const uint64_t* tomb = t->dead.empty() ? nullptr : t->d_tomb;
    d.d_deg = (uint32_t*)scratch.get(rows * sizeof(uint32_t));
    d.d_words = (unsigned long long*)scratch.get(DW_WORDS * sizeof(unsigned long long));
    HIP_CHECK(hipMemsetAsync(d.d_deg, 0, rows * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(d.d_words, 0, DW_WORDS * sizeof(unsigned long long), s));
    const bool pairs_possible = rows >= 2;
    WindowCall w;
    // the call's figures: mi_knn_dbscan_stats' words, or mi_knn_window_stats' (the tile and launch words are window_stage1's)
    auto keep_stats = [&] {
        if (!window) {
            for (int i = 0; i < 8; ++i) t->dbscan_stats[i] = d.stats[i];
            return;
        }
        w.stats[WS_CAND1] = d.stats[0]; w.stats[WS_WITHIN] = d.stats[1]; w.stats[WS_CAND2] = d.stats[3];
        for (int i = 0; i < WS_WORDS; ++i) t->window_stats[i] = w.stats[i];
    };
    if (pairs_possible) {
        const TableMirror tm = table_mirror(t, s, scratch);
        DensityStage1<true>& st = d.st1;
        st.s = s;
        st.a = st.b = DensitySide{tm.mirror, tm.xx, tm.tomb, n_rows, nullptr};
        st.blocks = &d.blocks; st.cross = nullptr;
        st.c = 1.0f - (max_dist + eps2(t->dim));
        st.cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
        st.d_cand = (uint2*)scratch.get((size_t)st.cand_cap * sizeof(uint2));
        st.d_count = d.d_words + DW_CAND;
        st.stats = d.stats;
        if (window) {
            w.s = s; w.dim = t->dim; w.n_rows = n_rows; w.first_new = 0;
            w.mirror = tm.mirror; w.xx = tm.xx; w.tomb = tm.tomb;
            w.c = st.c; w.cand_cap = st.cand_cap; w.d_cand = st.d_cand; w.d_count = st.d_count;
            window_ranges(t, s, scratch, *window, &w);
            d.win = &w;
        }
        dispatch_nch(t->dim, [&](auto nch) { d.template pass<decltype(nch)::value, 1>(); });
    }

    unsigned long long words[DW_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (min_pts == 0) {
        read_back(&out->counts, d.d_deg, rows, s);
        HIP_CHECK(hipMemcpyAsync(words, d.d_words, sizeof words, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        d.stats[1] = words[DW_WITHIN];
        keep_stats();
        return;
    }

    d.d_parent = (uint32_t*)scratch.get(rows * sizeof(uint32_t));
    d.d_bkey = (unsigned long long*)scratch.get(rows * sizeof(unsigned long long));
    d.d_act = (uint8_t*)scratch.get(d.n_blocks);
    hipLaunchKernelGGL(density_blocks_kernel, dim3(d.n_blocks), dim3(TILE), 0, s, d.d_deg, tomb, n_rows, min_pts, d.d_parent, d.d_bkey, d.d_act);
    HIP_CHECK(hipGetLastError());
    if (pairs_possible) {
        // the activity bytes, read back once: the host counts from them what the tiles of pass 2 do
        d.blocks.act.resize(d.n_blocks);
        HIP_CHECK(hipMemcpyAsync(d.blocks.act.data(), d.d_act, d.n_blocks, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        d.blocks.index();
        d.st1.a.act = d.st1.b.act = d.d_act;
        if (window) { w.blocks.act = d.blocks.act; w.d_act = d.d_act; }
        dispatch_nch(t->dim, [&](auto nch) { d.template pass<decltype(nch)::value, 2>(); });
    }

    uint64_t* d_cluster = (uint64_t*)scratch.get(rows * sizeof(uint64_t));
    uint64_t* d_via = want_via ? (uint64_t*)scratch.get(rows * sizeof(uint64_t)) : nullptr;
    float* d_via_dist = want_via_dist ? (float*)scratch.get(rows * sizeof(float)) : nullptr;
    const IdMap map = knn_id_map(t);
    hipLaunchKernelGGL(density_finish_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, d.d_deg, d.d_parent, d.d_bkey, tomb, n_rows,
                       min_pts, map, d_cluster, d_via, d_via_dist, d.d_words);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(words, d.d_words, sizeof words, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (words[DW_ERROR] != 0)
        fail(MI_ERR_HIP, "internal error: a step cap of the disjoint-set forest expired (%llu times); nothing was written",
             (unsigned long long)words[DW_ERROR]);
    read_back(&out->cluster, d_cluster, rows, s);
    if (want_via) read_back(&out->via, d_via, rows, s);
    if (want_via_dist) read_back(&out->via_dist, d_via_dist, rows, s);
    if (want_counts) read_back(&out->counts, d.d_deg, rows, s);   // (a deleted row is in no pair: its degree is the 0 the contract names)
    HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) out->summary[i] = words[DW_SUMMARY + i];
    d.stats[1] = words[DW_WITHIN];
    d.stats[6] = words[DW_MERGED];
    keep_stats();
}

// the public calls, each once for its plain and its windowed form (window null: the plain one)
int density_call(mi_knn* t, float max_dist, const uint64_t* window, uint32_t* counts) {
    return guarded([&] {
        const char* why = "";
        const int bad = density_check_args(t, max_dist, counts, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        DensityOut out;
        density_run(t, max_dist, 0, false, false, true, &out, window);
        copy_out(out.counts, counts);
    });
}

int dbscan_call(mi_knn* t, float max_dist, const uint64_t* window, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist,
                uint32_t* counts, uint64_t summary[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = dbscan_check_args(t, max_dist, min_pts, cluster, summary, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        DensityOut out;
        density_run(t, max_dist, min_pts, via != nullptr, via_dist != nullptr, counts != nullptr, &out, window);
        copy_out(out.cluster, cluster);
        copy_out(out.via, via);
        copy_out(out.via_dist, via_dist);
        copy_out(out.counts, counts);
        for (int i = 0; i < 4; ++i) summary[i] = out.summary[i];
    });
}

int themes_call(mi_index* ix, float max_dist, const uint64_t* window, uint32_t min_pts, uint64_t* ids, uint64_t cap_ids,
                uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups, uint64_t* n_noise) {
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
        density_run(t, max_dist, min_pts, false, false, false, &out, window);
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

}  // namespace

extern "C" {

int mi_knn_density(mi_knn* t, float max_dist, uint32_t* counts) { return density_call(t, max_dist, nullptr, counts); }

int mi_knn_density_window(mi_knn* t, float max_dist, uint64_t window, uint32_t* counts) { return density_call(t, max_dist, &window, counts); }

int mi_knn_dbscan(mi_knn* t, float max_dist, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist, uint32_t* counts,
                  uint64_t summary[4]) {
    return dbscan_call(t, max_dist, nullptr, min_pts, cluster, via, via_dist, counts, summary);
}

int mi_knn_dbscan_window(mi_knn* t, float max_dist, uint64_t window, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist,
                         uint32_t* counts, uint64_t summary[4]) {
    return dbscan_call(t, max_dist, &window, min_pts, cluster, via, via_dist, counts, summary);
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
    return themes_call(ix, max_dist, nullptr, min_pts, ids, cap_ids, group_start, cap_groups, n_ids, n_groups, n_noise);
}

int mi_index_events(mi_index* ix, float max_dist, uint64_t window, uint32_t min_pts, uint64_t* ids, uint64_t cap_ids,
                    uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups, uint64_t* n_noise) {
    return themes_call(ix, max_dist, &window, min_pts, ids, cap_ids, group_start, cap_groups, n_ids, n_groups, n_noise);
}

}  // extern "C"

