// join.hip — host side of the threshold self-join (mi_knn_near_pairs, mi_pairs_to_groups, mi_index_duplicates) and of its
// windowed form (mi_knn_near_pairs_window, mi_index_bursts: the same call with window.hip's stage 1).
// The kernels and the bound that makes the bf16 first stage exact: join_kernels.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "join_between_host.h"
#include "join_kernels.h"
#include "two_stage.h"
#include "window_call.h"

using namespace mi;

namespace {

struct Join {
    mi_knn* t;
    hipStream_t s;
    const uint16_t* mirror;
    const float* xx;
    const uint64_t* tomb;
    uint32_t n_rows, first_new, n_blocks;
    float max_dist, c;
    uint32_t cand_cap;
    uint64_t user_cap;
    uint2 *d_cand, *d_pairs;
    float* d_dist;
    unsigned long long* d_count;   // [0]: candidates of the strip, [1] (low word): pairs stage 2 kept
    std::vector<uint2> h_pairs;
    std::vector<float> h_dist;
    std::vector<JoinPair> out;
    uint64_t stats[4] = {0, 0, 0, 0};
    bool over = false;
    WindowCall* win = nullptr;     // the windowed join: stage 1 is window.hip's (it keeps the tile and launch counts)

    // The join's stages for rect_stages (two_stage.h).  Its tiles lie on or above the diagonal: bc0 is raised to br0, the
    // grid is two-dimensional and the tiles counted are the triangle's; once more than user_cap pairs qualify nothing more
    // is launched (checked between launches: the call stops there).
    template <int NCH>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) -> unsigned long long {
            c0 = std::max(c0, r0);
            if (over || c0 >= c1) return 0;
            if (win) return window_stage1(*win, 1, r0, r1, c0, c1);
            static DevOnce once;
            allow_lds_once(once, join_tiles_kernel<NCH>, JOIN_LDS);
            HIP_CHECK(hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), s));
            hipLaunchKernelGGL((join_tiles_kernel<NCH>), dim3(c1 - c0, r1 - r0), dim3(256), JOIN_LDS, s, mirror, xx, tomb, n_rows,
                               first_new, r0, c0, c, cand_cap, d_cand, d_count);
            HIP_CHECK(hipGetLastError());
            ++stats[2];
            for (uint32_t bi = r0; bi < r1; ++bi) stats[3] += c1 - std::max(c0, bi);
            return read_count(d_count, s);
        };
        auto stage2 = [&](uint32_t C) {
            stats[0] += C;
            hipLaunchKernelGGL((join_rescore_kernel<NCH>), dim3(group16_blocks(t, C)), dim3(256), 0, s, t->table, d_cand, C, max_dist,
                               d_pairs, d_dist, reinterpret_cast<uint32_t*>(d_count + 1));
            HIP_CHECK(hipGetLastError());
            uint32_t kept = 0;
            HIP_CHECK(hipMemcpyAsync(&kept, d_count + 1, sizeof kept, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (kept) {
                h_pairs.resize(kept);
                h_dist.resize(kept);
                HIP_CHECK(hipMemcpyAsync(h_pairs.data(), d_pairs, (size_t)kept * sizeof(uint2), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipMemcpyAsync(h_dist.data(), d_dist, (size_t)kept * sizeof(float), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                const size_t at = out.size();
                out.resize(at + kept);
                for (uint32_t j = 0; j < kept; ++j) out[at + j] = JoinPair{h_pairs[j].x, h_pairs[j].y, h_dist[j]};
            }
            stats[1] += kept;
            if (stats[1] > user_cap) over = true;
        };
        rect_stages(br0, br1, bc0, bc1, cand_cap, overflowed, stage1, stage2);
    }

    template <int NCH>
    void run() {
        // column blocks below first_new / TILE hold no b >= first_new
        tile_strips(0, n_blocks, first_new / TILE, n_blocks,
                    [&](uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) { rect<NCH>(br0, br1, bc0, bc1, overflowed); },
                    [&] { return over; });
    }
};

// first_new (an id of the table, one past its last id, or 0 = everything) -> local row
uint32_t local_first_new(const mi_knn* t, uint64_t first_new) {
    if (first_new == 0) return 0;
    const IdMap map = knn_id_map(t);
    if (first_new == id_of_local(map, t->rows)) return (uint32_t)t->rows;
    // (ids are monotone in the local ordinal: a binary search serves the plain and the block-cyclic map alike)
    uint64_t lo = 0, hi = t->rows;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (id_of_local(map, mid) < first_new) lo = mid + 1; else hi = mid;
    }
    if (lo >= t->rows || id_of_local(map, lo) != first_new)
        fail(MI_ERR_INVALID, "first_new %llu is neither a row of this table (base %llu, %llu rows) nor one past its last",
             (unsigned long long)first_new, (unsigned long long)t->base, (unsigned long long)t->rows);
    return (uint32_t)lo;
}

// the join itself: pairs as local rows, ascending by (a, b); *over = more than user_cap pairs qualify (out is then partial).
// first_new_id: an id (local_first_new), or with first_new_is_local the local row itself (what a shard of the sharded join is
// handed: the number of its rows below the global bound)
// window (nullable): only the pairs whose stamps lie within *window of each other (W_win); the call's figures then go to
// t->window_stats and t->join_stats stays as it is
void near_pairs(mi_knn* t, float max_dist, uint64_t first_new_id, uint64_t user_cap, std::vector<JoinPair>* out, bool* over,
                bool first_new_is_local = false, const uint64_t* window = nullptr) {
    out->clear();
    *over = false;
    std::lock_guard<std::mutex> l(t->mu);
    if (window) std::fill(std::begin(t->window_stats), std::end(t->window_stats), 0);
    else std::fill(std::begin(t->join_stats), std::end(t->join_stats), 0);
    const uint32_t fn = first_new_is_local ? (uint32_t)std::min<uint64_t>(first_new_id, t->rows) : local_first_new(t, first_new_id);
    check_mirror_dim(t->dim, "the join's");
    if (t->rows < 2 || fn >= t->rows) return;
    Scratch scratch;
    TableCall call(t);
    hipStream_t s = call.s;
    Join j;
    j.t = t; j.s = s;
    j.n_rows = (uint32_t)t->rows; j.first_new = fn;
    j.n_blocks = (uint32_t)((t->rows + TILE - 1) / TILE);
    j.max_dist = max_dist;
    j.c = 1.0f - (max_dist + eps2(t->dim));
    j.cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
    j.user_cap = user_cap;
    const TableMirror tm = table_mirror(t, s, scratch);
    j.mirror = tm.mirror; j.xx = tm.xx; j.tomb = tm.tomb;
    j.d_cand = (uint2*)scratch.get((size_t)j.cand_cap * sizeof(uint2));
    j.d_pairs = (uint2*)scratch.get((size_t)j.cand_cap * sizeof(uint2));
    j.d_dist = (float*)scratch.get((size_t)j.cand_cap * sizeof(float));
    j.d_count = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
    WindowCall w;
    if (window) {
        w.s = s; w.dim = t->dim; w.n_rows = j.n_rows; w.first_new = fn;
        w.mirror = tm.mirror; w.xx = tm.xx; w.tomb = tm.tomb;
        w.c = j.c; w.cand_cap = j.cand_cap; w.d_cand = j.d_cand; w.d_count = j.d_count; w.count_words = 2;
        window_ranges(t, s, scratch, *window, &w);
        j.win = &w;
    }

    dispatch_nch(t->dim, [&](auto nch) { j.template run<decltype(nch)::value>(); });
    if (window) {
        w.stats[WS_CAND1] = j.stats[0]; w.stats[WS_WITHIN] = j.stats[1];
        for (int i = 0; i < WS_WORDS; ++i) t->window_stats[i] = w.stats[i];
    } else {
        for (int i = 0; i < 4; ++i) t->join_stats[i] = j.stats[i];
    }
    *over = j.over;
    if (j.over) return;
    std::sort(j.out.begin(), j.out.end(), [](const JoinPair& x, const JoinPair& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    out->swap(j.out);
}

void check_join_args(const mi_knn* t, float max_dist) {
    if (!(max_dist >= 0.0f)) fail(MI_ERR_INVALID, "max_dist must be a number >= 0 (got %g)", (double)max_dist);
    if (!t) fail(MI_ERR_INVALID, "null table handle");
}

// pairs -> connected components.  ids_out: every id of a pair, grouped; starts: n_groups + 1 offsets into it
void groups_of(const uint64_t* a, const uint64_t* b, uint64_t n_pairs, std::vector<uint64_t>* ids_out, std::vector<uint64_t>* starts) {
    std::vector<uint64_t> ids;
    ids.reserve((size_t)n_pairs * 2);
    for (uint64_t i = 0; i < n_pairs; ++i) { ids.push_back(a[i]); ids.push_back(b[i]); }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const size_t n = ids.size();
    std::vector<uint32_t> parent(n);
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    auto slot = [&](uint64_t id) { return (uint32_t)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
    for (uint64_t i = 0; i < n_pairs; ++i) {
        const uint32_t x = find(slot(a[i])), y = find(slot(b[i]));
        if (x != y) parent[std::max(x, y)] = std::min(x, y);   // the root is the component's smallest id
    }
    // groups ordered by their smallest id (= their root), ids ascending inside: a stable counting pass over the sorted ids
    std::vector<uint32_t> root(n), order;
    std::vector<uint64_t> size(n, 0);
    for (size_t i = 0; i < n; ++i) { root[i] = find((uint32_t)i); ++size[root[i]]; }
    std::vector<uint64_t> at(n, 0);
    starts->clear();
    uint64_t run = 0;
    for (size_t i = 0; i < n; ++i)
        if (root[i] == i) { at[i] = run; starts->push_back(run); run += size[i]; }
    starts->push_back(run);
    ids_out->assign(n, 0);
    for (size_t i = 0; i < n; ++i) (*ids_out)[at[root[i]]++] = ids[i];
}

void write_groups(const std::vector<uint64_t>& gids, const std::vector<uint64_t>& starts, uint64_t* ids, uint64_t cap_ids,
                  uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups) {
    *n_ids = gids.size();
    *n_groups = starts.size() - 1;
    if (ids) std::copy(gids.begin(), gids.begin() + (size_t)std::min<uint64_t>(cap_ids, gids.size()), ids);
    if (group_start) std::copy(starts.begin(), starts.begin() + (size_t)std::min<uint64_t>(cap_groups, starts.size()), group_start);
}

}  // namespace

namespace mi {
void knn_near_pairs_local(mi_knn* t, float max_dist, uint64_t first_new_local, uint64_t user_cap, std::vector<JoinPair>* out, bool* over) {
    near_pairs(t, max_dist, first_new_local, user_cap, out, over, true);
}
}  // namespace mi

extern "C" {

// mi_knn_near_pairs (window null) and mi_knn_near_pairs_window: one contract, W or W_win
static int near_pairs_call(mi_knn* t, float max_dist, const uint64_t* window, uint64_t first_new, uint64_t* a, uint64_t* b, float* dist,
                           uint64_t cap, uint64_t* count) {
    return guarded([&] {
        if (count) *count = 0;
        check_join_args(t, max_dist);
        if (!count) fail(MI_ERR_INVALID, "count is null");
        if (cap && (!a || !b || !dist)) fail(MI_ERR_INVALID, "a, b or dist is null with cap %llu", (unsigned long long)cap);
        std::vector<JoinPair> pairs;
        bool over = false;
        near_pairs(t, max_dist, first_new, cap, &pairs, &over, false, window);
        if (over) {
            *count = cap + 1;
            fail(MI_ERR_UNSUPPORTED, "more than %llu pairs lie within %g: lower max_dist or raise cap", (unsigned long long)cap,
                 (double)max_dist);
        }
        const IdMap map = knn_id_map(t);
        for (size_t i = 0; i < pairs.size(); ++i) {
            a[i] = id_of_local(map, pairs[i].a);
            b[i] = id_of_local(map, pairs[i].b);
            dist[i] = pairs[i].d;
        }
        *count = pairs.size();
    });
}

int mi_knn_near_pairs(mi_knn* t, float max_dist, uint64_t first_new, uint64_t* a, uint64_t* b, float* dist, uint64_t cap,
                      uint64_t* count) {
    return near_pairs_call(t, max_dist, nullptr, first_new, a, b, dist, cap, count);
}

int mi_knn_near_pairs_window(mi_knn* t, float max_dist, uint64_t window, uint64_t first_new, uint64_t* a, uint64_t* b, float* dist,
                             uint64_t cap, uint64_t* count) {
    return near_pairs_call(t, max_dist, &window, first_new, a, b, dist, cap, count);
}

int mi_knn_near_pairs_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->join_stats[i];
    });
}

int mi_pairs_to_groups(const uint64_t* a, const uint64_t* b, uint64_t n_pairs, uint64_t* ids, uint64_t cap_ids, uint64_t* group_start,
                       uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups) {
    return guarded([&] {
        if (!n_ids || !n_groups) fail(MI_ERR_INVALID, "n_ids or n_groups is null");
        *n_ids = 0; *n_groups = 0;
        if (n_pairs && (!a || !b)) fail(MI_ERR_INVALID, "a or b is null with %llu pairs", (unsigned long long)n_pairs);
        if ((cap_ids && !ids) || (cap_groups && !group_start)) fail(MI_ERR_INVALID, "an output array is null with a cap > 0");
        if (n_pairs >= (1ull << 31)) fail(MI_ERR_UNSUPPORTED, "at most 2^31 - 1 pairs (got %llu)", (unsigned long long)n_pairs);
        std::vector<uint64_t> gids, starts;
        groups_of(a, b, n_pairs, &gids, &starts);
        write_groups(gids, starts, ids, cap_ids, group_start, cap_groups, n_ids, n_groups);
    });
}

// mi_index_duplicates (window null) and mi_index_bursts: the components of W or of W_win
static int duplicates_call(mi_index* ix, float max_dist, const uint64_t* window, uint64_t first_new, uint64_t max_pairs, uint64_t* ids,
                           uint64_t cap_ids, uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups) {
    return guarded([&] {
        if (n_ids) *n_ids = 0;
        if (n_groups) *n_groups = 0;
        if (!ix) fail(MI_ERR_INVALID, "null index handle");
        mi_knn* t = mi_index_table(ix);
        check_join_args(t, max_dist);
        if (!n_ids || !n_groups) fail(MI_ERR_INVALID, "n_ids or n_groups is null");
        if ((cap_ids && !ids) || (cap_groups && !group_start)) fail(MI_ERR_INVALID, "an output array is null with a cap > 0");
        std::vector<JoinPair> pairs;
        bool over = false;
        // (a removed path's rows are deleted rows of the table: the join never reports them)
        near_pairs(t, max_dist, first_new, max_pairs, &pairs, &over, false, window);
        if (over)
            fail(MI_ERR_UNSUPPORTED, "more than %llu pairs lie within %g: lower max_dist or raise max_pairs",
                 (unsigned long long)max_pairs, (double)max_dist);
        const IdMap map = knn_id_map(t);
        std::vector<uint64_t> pa(pairs.size()), pb(pairs.size());
        for (size_t i = 0; i < pairs.size(); ++i) { pa[i] = id_of_local(map, pairs[i].a); pb[i] = id_of_local(map, pairs[i].b); }
        std::vector<uint64_t> gids, starts;
        groups_of(pa.data(), pb.data(), pairs.size(), &gids, &starts);
        write_groups(gids, starts, ids, cap_ids, group_start, cap_groups, n_ids, n_groups);
    });
}

int mi_index_duplicates(mi_index* ix, float max_dist, uint64_t first_new, uint64_t max_pairs, uint64_t* ids, uint64_t cap_ids,
                        uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups) {
    return duplicates_call(ix, max_dist, nullptr, first_new, max_pairs, ids, cap_ids, group_start, cap_groups, n_ids, n_groups);
}

int mi_index_bursts(mi_index* ix, float max_dist, uint64_t window, uint64_t first_new, uint64_t max_pairs, uint64_t* ids,
                    uint64_t cap_ids, uint64_t* group_start, uint64_t cap_groups, uint64_t* n_ids, uint64_t* n_groups) {
    return duplicates_call(ix, max_dist, &window, first_new, max_pairs, ids, cap_ids, group_start, cap_groups, n_ids, n_groups);
}

}  // extern "C"
