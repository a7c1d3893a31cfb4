// sharded_calls.hip — the calls on the sharded table (sharded.hip) that scatter to the shards and merge on the host, all on the
// frame of sharded_call.h: the compound, paged, ordered and grouped searches and the stamp histogram on global ids, the
// predicate count, and the columns every shard keeps for its own rows (deleted rows, groups, attributes).  A shard is an mi_knn
// whose ids are the global ones (base 0, the block-cyclic map), so its lists merge with the single table's ordering.
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "compound_host.h"
#include "grouped_host.h"
#include "handles.h"
#include "ordered_host.h"
#include "page_host.h"
#include "sharded_call.h"
#include "where_host.h"

using namespace mi;

namespace {

// the cursor's row of a paged or ordered search; t->mu held
void check_after_id(const mi_knn_sharded* t, uint64_t after_id) {
    if (after_id >= t->rows)
        fail(MI_ERR_INVALID, "after_id %llu is not a row of this table (%llu rows)", (unsigned long long)after_id, (unsigned long long)t->rows);
}

}  // namespace

namespace mi {

// the predicate's count = the shards' counts summed
uint64_t sharded_count_where(mi_knn_sharded* t, const mi_knn_where* w) {
    uint64_t sum = 0;
    for (mi_knn* sh : t->shard) {
        uint64_t one = 0;
        call_ok(mi_knn_count_where(sh, w, &one));
        sum += one;
    }
    return sum;
}

// ---- the columns: every id checked first (a call with one bad id writes nothing), then each shard takes its own ids ----------
uint64_t sharded_delete(mi_knn_sharded* t, const uint64_t* ids, uint64_t n) {
    uint64_t newly = 0;
    route_ids(t, ids, n, NULL_IS_NO_LIST).each([&](uint32_t s, const auto& mine, const auto&) {
        uint64_t m = 0;
        call_ok(mi_knn_delete(t->shard[s], mine.data(), mine.size(), &m));
        newly += m;
    });
    return newly;
}
std::vector<uint64_t> sharded_deleted(mi_knn_sharded* t) {
    std::vector<uint64_t> all;
    for (mi_knn* sh : t->shard) {
        uint64_t c = 0;
        call_ok(mi_knn_deleted(sh, nullptr, 0, &c), MI_ERR_INVALID);
        const size_t at = all.size();
        all.resize(at + c);
        if (c) call_ok(mi_knn_deleted(sh, all.data() + at, c, &c), MI_ERR_INVALID);
    }
    std::sort(all.begin(), all.end());
    return all;
}
// the group column (grouped.hip).  ids == nullptr: the first n global rows
void sharded_set_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint32_t* groups) {
    const uint64_t bad = grouped_first_bad(groups, n);   // before any shard is written
    if (bad < n) fail(MI_ERR_INVALID, "group id %u (entry %llu) is neither below 2^24 nor MI_KNN_NO_GROUP", groups[bad], (unsigned long long)bad);
    route_ids(t, ids, n, NULL_IS_FIRST_ROWS).each([&](uint32_t s, const auto& mine, const auto& at) {
        std::vector<uint32_t> g(mine.size());
        for (size_t i = 0; i < mine.size(); ++i) g[i] = groups[at[i]];
        call_ok(mi_knn_set_groups(t->shard[s], mine.data(), mine.size(), g.data()));
    });
}
void sharded_get_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint32_t* groups) {
    route_ids(t, ids, n, NULL_IS_FIRST_ROWS).each([&](uint32_t s, const auto& mine, const auto& at) {
        std::vector<uint32_t> g(mine.size());
        call_ok(mi_knn_get_groups(t->shard[s], mine.data(), mine.size(), g.data()));
        for (size_t i = 0; i < mine.size(); ++i) groups[at[i]] = g[i];
    });
}
void sharded_groups_info(mi_knn_sharded* t, uint64_t info[2]) {
    info[0] = info[1] = 0;
    for (mi_knn* sh : t->shard) {
        uint64_t one[2] = {0, 0};
        call_ok(mi_knn_groups_info(sh, one));
        info[0] = std::max(info[0], one[0]);
        info[1] += one[1];
    }
}
// the attribute columns (where.hip): the same routing.  A column that is null is neither written nor read
void sharded_set_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint64_t* tags, const int64_t* stamps) {
    route_ids(t, ids, n, NULL_IS_FIRST_ROWS).each([&](uint32_t s, const auto& mine, const auto& at) {
        std::vector<uint64_t> tg(tags ? mine.size() : 0);
        std::vector<int64_t> st(stamps ? mine.size() : 0);
        for (size_t i = 0; i < mine.size(); ++i) {
            if (tags) tg[i] = tags[at[i]];
            if (stamps) st[i] = stamps[at[i]];
        }
        call_ok(mi_knn_set_attrs(t->shard[s], mine.data(), mine.size(), tags ? tg.data() : nullptr, stamps ? st.data() : nullptr));
    });
}
void sharded_get_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint64_t* tags, int64_t* stamps) {
    route_ids(t, ids, n, NULL_IS_FIRST_ROWS).each([&](uint32_t s, const auto& mine, const auto& at) {
        std::vector<uint64_t> tg(mine.size());
        std::vector<int64_t> st(mine.size());
        call_ok(mi_knn_get_attrs(t->shard[s], mine.data(), mine.size(), tg.data(), st.data()));
        for (size_t i = 0; i < mine.size(); ++i) {
            if (tags) tags[at[i]] = tg[i];
            if (stamps) stamps[at[i]] = st[i];
        }
    });
}

}  // namespace mi

extern "C" {

// the predicate calls on global ids (where.hip); mi_knn_sharded_search_where: sharded.hip
int mi_knn_sharded_count_where(mi_knn_sharded* t, const mi_knn_where* w, uint64_t* count) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_rows_args(t, w, nullptr, 0, count, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        ShardedCall call(t);
        call.ready();
        *count = sharded_count_where(t, w);
    });
}

// mi_knn_search_compound on global ids: every shard answers for the rows (the ids of `among`) it holds, on its own stream and
// host thread; the lists carry global ids and are merged with mi_knn_merge's ordering
int mi_knn_sharded_search_compound(mi_knn_sharded* t, const float* pos, uint32_t n_pos, int mode, const float* neg,
                                   const float* neg_within, uint32_t n_neg, uint32_t k, const uint64_t* among, uint64_t n_among,
                                   uint64_t* idx, float* dist) {
    return guarded([&] {
        const char* why = "";
        const int bad = compound_check_args(t, pos, n_pos, mode, neg, neg_within, n_neg, k, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (n_pos %u, n_neg %u, mode %d, k %u)", why, n_pos, n_neg, mode, k);
        ShardedCall call(t, among, n_among);
        ShardLists<> all(call.n, 1, k);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            knn_search_compound(sh, pos, n_pos, mode, neg, neg_within, n_neg, k, call.ids.of(si), call.ids.n_of(si), all.idx(si), all.dist(si),
                                nullptr);
        });
        merge_shard_lists(all, idx, dist);
    });
}

// mi_knn_search_page on global ids: every shard answers for the rows (the ids of `among`) it holds, on its own stream and host
// thread.  A shard's local rows ascend with their global ids, so its window opens at (after_dist, the number of its rows whose
// global id is <= after_id) — page_host.h; the lists carry global ids and are merged with mi_knn_merge's ordering, the counts
// are summed
int mi_knn_sharded_search_page(mi_knn_sharded* t, const float* q, uint32_t k, float after_dist, uint64_t after_id, float max_dist,
                               const uint64_t* among, uint64_t n_among, uint64_t* idx, float* dist, uint64_t counts[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = page_check_args(t, q, k, after_dist, after_id, max_dist, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        ShardedCall call(t, among, n_among);
        if (after_id != MI_KNN_NO_ID) check_after_id(t, after_id);
        ShardLists<> all(call.n, 1, k, 4);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            const uint64_t first_key = after_id == MI_KNN_NO_ID ? 0 : page_first_key_at(after_dist, sharded_rows_of(t, after_id + 1, si));
            knn_search_page(sh, q, k, false, 0.0f, MI_KNN_NO_ID, first_key, max_dist, call.ids.of(si), call.ids.n_of(si), all.idx(si),
                            all.dist(si), all.counts(si));
        });
        merge_shard_lists(all, idx, dist);
        if (counts) all.sum_counts(counts);
    });
}

// mi_knn_search_ordered on global ids: every shard runs the call on its own rows, on its own stream and host thread.  A shard's
// local rows ascend with their global ids, so its cursor is (okey(after_stamp), the number of its rows whose global id is <=
// after_id) — ordered_host.h; the lists carry global ids and stamps and are merged by (okey, id), the counts are summed
int mi_knn_sharded_search_ordered(mi_knn_sharded* t, const float* q, uint32_t k, float max_dist, const mi_knn_where* w, uint32_t flags,
                                  int64_t after_stamp, uint64_t after_id, uint64_t* idx, float* dist, int64_t* stamps, uint64_t counts[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = ordered_check_args(t, q, k, max_dist, w, flags, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        ShardedCall call(t);
        if (flags & MI_KNN_ORDER_AFTER) check_after_id(t, after_id);
        ShardLists<int64_t> all(call.n, 1, k, 4, true);   // the further column: the stamps
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            const OrderedCursor cur = ordered_cursor_shard(t->block, call.n, si, flags, after_stamp, after_id);
            knn_search_ordered(sh, q, k, max_dist, w, flags, after_stamp, after_id, &cur, all.idx(si), all.dist(si), all.extra(si),
                               all.counts(si));
        });
        // (the merge writes only once nothing can fail any more: straight into the caller's arrays)
        ordered_merge(all.idx(0), all.dist(0), all.extra(0), call.n, k, (flags & MI_KNN_ORDER_DESC) != 0, idx, dist, stamps);
        if (counts) all.sum_counts(counts);
    });
}

// mi_knn_stamp_histogram over all shards: every shard counts its own rows, the host sums the bins
int mi_knn_sharded_stamp_histogram(mi_knn_sharded* t, const float* q, float max_dist, const mi_knn_where* w, const int64_t* edges,
                                   uint32_t n_edges, uint64_t* hist) {
    return guarded([&] {
        const char* why = "";
        const int bad = ordered_check_hist_args(t, q, max_dist, w, edges, n_edges, hist, &why);
        if (bad != MI_OK) fail(bad, "%s (n_edges %u)", why, n_edges);
        ShardedCall call(t);
        ShardLists<> all(call.n, 0, 0, (size_t)n_edges + 1);   // no lists: the bins are the counters
        call.for_each_shard([&](uint32_t si, mi_knn* sh) { knn_stamp_histogram(sh, q, max_dist, w, edges, n_edges, all.counts(si)); });
        all.sum_counts(hist);
    });
}

// mi_knn_search_grouped on global ids: every shard answers with its k best representatives (global ids, its own column); the
// host merges them by group id (grouped_host.h: grouped_merge).  members of the winners: every shard gathers its counts of the
// k winning groups on the device, the host sums k words per shard.  facets / totals[0] need the shards' whole count arrays.
int mi_knn_sharded_search_grouped(mi_knn_sharded* t, const float* q, uint32_t k, float max_dist, const uint64_t* among,
                                  uint64_t n_among, uint64_t* idx, float* dist, uint32_t* group, uint64_t* members,
                                  uint64_t* facets, uint64_t cap_facets, uint64_t totals[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = grouped_check_args(t, q, k, max_dist, among, n_among, idx, dist, &why);
        if (bad != MI_OK) fail(bad, "%s (k %u)", why, k);
        ShardedCall call(t);
        const uint32_t n = call.n;
        uint64_t n_groups = 0;
        for (mi_knn* sh : t->shard) {
            std::lock_guard<std::mutex> ls(sh->mu);
            n_groups = std::max<uint64_t>(n_groups, sh->n_groups);
        }
        if (facets && cap_facets < n_groups)
            fail(MI_ERR_INVALID, "facets holds %llu entries, the table has %llu groups", (unsigned long long)cap_facets, (unsigned long long)n_groups);
        call.route(among, n_among);
        const bool sums = facets || totals;
        ShardLists<uint32_t> all(n, 1, k, 4, true);   // the further column: the groups
        std::vector<std::vector<uint32_t>> cnt(n);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            knn_search_grouped(sh, q, k, max_dist, call.ids.of(si), call.ids.n_of(si), all.idx(si), all.dist(si), all.extra(si), nullptr, nullptr,
                               0, all.counts(si), sums ? &cnt[si] : nullptr);
        });
        // (the members pass below may still fail: the winners wait in storage of the call's)
        std::vector<uint64_t> m_idx(k);
        std::vector<float> m_dist(k);
        std::vector<uint32_t> m_group(k);
        grouped_merge(all.idx(0), all.dist(0), all.extra(0), n, k, m_idx.data(), m_dist.data(), m_group.data());
        if (members) {
            std::vector<uint32_t> part((size_t)n * k, 0);
            call.for_each_shard([&](uint32_t si, mi_knn* sh) { knn_grouped_members(sh, m_group.data(), k, part.data() + (size_t)si * k); });
            for (uint32_t j = 0; j < k; ++j) {
                uint64_t m = m_idx[j] == MI_KNN_NO_ID ? 0 : m_group[j] == MI_KNN_NO_GROUP ? 1 : 0;
                if (m_group[j] != MI_KNN_NO_GROUP)
                    for (uint32_t si = 0; si < n; ++si) m += part[(size_t)si * k + j];
                members[j] = m;
            }
        }
        std::copy(m_idx.begin(), m_idx.end(), idx);
        std::copy(m_dist.begin(), m_dist.end(), dist);
        if (group) std::copy(m_group.begin(), m_group.end(), group);
        if (sums) {
            std::vector<uint64_t> reps(n);
            for (uint32_t si = 0; si < n; ++si) reps[si] = all.counts(si)[0];
            const uint64_t total_reps = grouped_sum_counts(cnt, reps.data(), n_groups, facets);
            if (totals) {
                all.sum_counts(totals);
                totals[0] = total_reps;   // representatives are counted per group over all shards, not per shard
            }
        }
    });
}

// ---- the column calls: deleted rows, groups, attributes ----------------------------------------------------------------------
int mi_knn_sharded_delete(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint64_t* newly) {
    return guarded([&] {
        ShardedCall call(t);
        if (newly) *newly = 0;
        if (n == 0) return;
        if (!ids) fail(MI_ERR_INVALID, "ids is null");
        const uint64_t m = sharded_delete(t, ids, n);
        if (newly) *newly = m;
    });
}

int mi_knn_sharded_deleted(mi_knn_sharded* t, uint64_t* ids, uint64_t cap, uint64_t* count) {
    return guarded([&] {
        if (!t || !count) fail(MI_ERR_INVALID, "null argument");
        ShardedCall call(t);
        const std::vector<uint64_t> all = sharded_deleted(t);   // ascending
        *count = all.size();
        if (ids) std::copy(all.begin(), all.begin() + std::min<uint64_t>(cap, all.size()), ids);
    });
}

int mi_knn_sharded_set_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint32_t* groups) {
    return guarded([&] {
        ShardedCall call(t);
        if (n == 0) return;
        if (!groups) fail(MI_ERR_INVALID, "groups is null");
        sharded_set_groups(t, ids, n, groups);
    });
}

int mi_knn_sharded_get_groups(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint32_t* groups) {
    return guarded([&] {
        ShardedCall call(t);
        if (n == 0) return;
        if (!groups) fail(MI_ERR_INVALID, "groups is null");
        sharded_get_groups(t, ids, n, groups);
    });
}

int mi_knn_sharded_set_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, const uint64_t* tags, const int64_t* stamps) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_attrs_args(t, ids, n, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        if (n == 0 || (!tags && !stamps)) return;
        ShardedCall call(t);
        sharded_set_attrs(t, ids, n, tags, stamps);
    });
}

int mi_knn_sharded_get_attrs(mi_knn_sharded* t, const uint64_t* ids, uint64_t n, uint64_t* tags, int64_t* stamps) {
    return guarded([&] {
        const char* why = "";
        const int bad = where_check_attrs_args(t, ids, n, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        if (n == 0) return;
        ShardedCall call(t);
        sharded_get_attrs(t, ids, n, tags, stamps);
    });
}

int mi_knn_sharded_groups_info(mi_knn_sharded* t, uint64_t info[2]) {
    return guarded([&] {
        if (!t || !info) fail(MI_ERR_INVALID, "null argument");
        ShardedCall call(t);
        sharded_groups_info(t, info);
    });
}

}  // extern "C"
