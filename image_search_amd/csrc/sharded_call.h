// sharded_call.h — what the calls on the sharded table share on the host: the router that deals a list of global ids to the
// shards, the per-shard result lists with their counters, the merge of those lists, the frame of such a call (ShardedCall) and
// the thread per shard.  The per-call argument rules, cursors, merges by other keys and the counters that are not plain sums
// stay with the calls: they are the contracts.
//
// The first part holds rules without HIP in them; a host compiler sees that part alone (tests/cpp/test_sharded_call_host.cpp
// runs it under the sanitizers).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "error.h"
#include "ids.h"
#include "page_host.h"   // the search's key transform on the host

namespace mi {

// ---- global ids -> the shards that hold them ------------------------------------------------------------------------------
// what a null list means to the call: no list at all (every shard answers for all its rows), or the first n rows of the table
enum NullList { NULL_IS_NO_LIST, NULL_IS_FIRST_ROWS };

struct ShardRoute {
    std::vector<std::vector<uint64_t>> ids, at;   // [shard]: its ids in the list's order, and the positions they came from
    bool listed = false;                          // false: no list was given
    // what shard s's call takes: null = no list; a shard that holds none of the ids gets an empty candidate set, not "every row"
    const uint64_t* of(uint32_t s) const {
        static const uint64_t none = 0;
        return !listed ? nullptr : ids[s].empty() ? &none : ids[s].data();
    }
    uint64_t n_of(uint32_t s) const { return ids[s].size(); }
    // f(shard, its ids, their positions) for every shard that holds some
    template <class F>
    void each(F&& f) const {
        for (uint32_t s = 0; s < ids.size(); ++s)
            if (!ids[s].empty()) f(s, ids[s], at[s]);
    }
};
// Every id is checked against `rows` before any is dealt (a call with one bad id does nothing).
inline ShardRoute route_ids(uint32_t block, uint32_t n_shards, uint64_t rows, const uint64_t* ids, uint64_t n, NullList null_means) {
    ShardRoute r;
    r.ids.resize(n_shards);
    r.at.resize(n_shards);
    r.listed = ids != nullptr || null_means == NULL_IS_FIRST_ROWS;
    if (!r.listed) return r;
    if (!ids && n > rows) fail(MI_ERR_INVALID, "%llu rows asked of a table of %llu", (unsigned long long)n, (unsigned long long)rows);
    for (uint64_t i = 0; ids && i < n; ++i)
        if (ids[i] >= rows)
            fail(MI_ERR_INVALID, "id %llu is not a row of this table (%llu rows)", (unsigned long long)ids[i], (unsigned long long)rows);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t id = ids ? ids[i] : i;
        uint32_t s; uint64_t local;
        cyclic_place(block, n_shards, id, &s, &local);
        r.ids[s].push_back(id);
        r.at[s].push_back(i);
    }
    return r;
}

// ---- the lists the shards answer with --------------------------------------------------------------------------------------
// n shards x nq queries x k entries of (id, distance), optionally a further column of X per entry (stamps, groups), and n x C
// counters.  Shard si writes at idx(si) / dist(si) / extra(si) / counts(si); its lists lie [nq][k].
template <class X = char>
struct ShardLists {
    uint32_t n, nq, k;
    size_t C;
    std::vector<uint64_t> all_idx, all_counts;
    std::vector<float> all_dist;
    std::vector<X> all_extra;
    ShardLists(uint32_t n_shards, uint32_t n_queries, uint32_t k_each, size_t n_counters = 0, bool with_extra = false)
        : n(n_shards), nq(n_queries), k(k_each), C(n_counters), all_idx(per() * n), all_counts(C * n, 0), all_dist(per() * n),
          all_extra(with_extra ? per() * n : 0) {}
    size_t per() const { return (size_t)nq * k; }
    uint64_t* idx(uint32_t si) { return all_idx.data() + per() * si; }
    float* dist(uint32_t si) { return all_dist.data() + per() * si; }
    X* extra(uint32_t si) { return all_extra.data() + per() * si; }
    uint64_t* counts(uint32_t si) { return all_counts.data() + C * si; }
    // out[c] = the sum over the shards of counter c
    void sum_counts(uint64_t* out) const {
        for (size_t c = 0; c < C; ++c) {
            out[c] = 0;
            for (uint32_t si = 0; si < n; ++si) out[c] += all_counts[C * si + c];
        }
    }
};

// global top-k of `lists` candidate lists of k (id, distance) entries under (distance key asc, id asc) — page_dist_key, the
// 32-bit monotone image of the distance the kernels use: NaN last (mi_knn_merge)
inline void merge_lists(const uint64_t* idx_in, const float* dist_in, uint32_t lists, uint32_t k, uint64_t* idx, float* dist) {
    struct Ent { uint32_t key; uint64_t id; float d; };
    std::vector<Ent> all;
    all.reserve((size_t)lists * k);
    for (size_t i = 0; i < (size_t)lists * k; ++i)
        if (idx_in[i] != MI_KNN_NO_ID) all.push_back({page_dist_key(dist_in[i]), idx_in[i], dist_in[i]});
    const size_t keep = std::min<size_t>(k, all.size());
    std::partial_sort(all.begin(), all.begin() + keep, all.end(), [](const Ent& a, const Ent& b) {
        return a.key < b.key || (a.key == b.key && a.id < b.id);
    });
    for (uint32_t i = 0; i < k; ++i) {
        if (i < keep) { idx[i] = all[i].id; dist[i] = all[i].d; }
        else { idx[i] = MI_KNN_NO_ID; dist[i] = INFINITY; }
    }
}

// The shards' lists [shard][nq][k] -> idx / dist [nq][k] in merge_lists' ordering, query by query.  Merged into storage of its
// own and copied out at the end: a failure leaves idx / dist as they were.
template <class X>
void merge_shard_lists(const ShardLists<X>& all, uint64_t* idx, float* dist) {
    const uint32_t n = all.n, k = all.k;
    std::vector<uint64_t> li((size_t)n * k), m_idx(all.per());
    std::vector<float> ld((size_t)n * k), m_dist(all.per());
    for (uint32_t u = 0; u < all.nq; ++u) {
        for (uint32_t si = 0; si < n; ++si) {
            const size_t from = all.per() * si + (size_t)u * k;
            std::copy_n(all.all_idx.data() + from, k, li.data() + (size_t)si * k);
            std::copy_n(all.all_dist.data() + from, k, ld.data() + (size_t)si * k);
        }
        merge_lists(li.data(), ld.data(), n, k, m_idx.data() + (size_t)u * k, m_dist.data() + (size_t)u * k);
    }
    std::copy(m_idx.begin(), m_idx.end(), idx);
    std::copy(m_dist.begin(), m_dist.end(), dist);
}

}  // namespace mi

#ifdef __HIPCC__
#include <mutex>
#include <string>
#include <thread>
#include <utility>

#include "common.h"
#include "handles.h"

namespace mi {

// the router over a table's own layout; t->mu held
inline ShardRoute route_ids(const mi_knn_sharded* t, const uint64_t* ids, uint64_t n, NullList null_means) {
    return route_ids(t->block, t->n(), t->rows, ids, n, null_means);
}

// bytes between two shards' devices (the same one: a device-to-device copy), enqueued on s
inline void copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t s) {
    if (bytes == 0) return;
    if (dst_dev == src_dev) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    else HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s));
}

// job(i) for i < n, each on a host thread of its own (a shard's call reads its candidate counts back between launches); all
// are joined, then the first that failed goes to report(i, code, message), which throws.
template <class Job, class Report>
void fan_out(size_t n, Job&& job, Report&& report) {
    std::vector<int> codes(n, MI_OK);
    std::vector<std::string> msgs(n);
    std::vector<std::thread> threads;
    for (size_t i = 0; i < n; ++i) {
        threads.emplace_back([&, i] {
            try {
                job(i);
            } catch (const Error& e) {
                codes[i] = e.code; msgs[i] = e.what();
            } catch (const std::exception& e) {
                codes[i] = MI_ERR_INVALID; msgs[i] = e.what();
            }
        });
    }
    for (std::thread& th : threads) th.join();
    for (size_t i = 0; i < n; ++i)
        if (codes[i] != MI_OK) report(i, codes[i], msgs[i].c_str());
}

// The frame of a call on the sharded table: t->mu held until it leaves, a table that has no shard refused, an optional list of
// global ids checked and dealt to the shards (`ids`).  What the call checks under the lock comes next; then ready() delivers
// the searches still pending in the ring, in front of the first touch of a shard.  Every failure of an argument is therefore
// raised with the ring and the shards untouched.  The fan-outs call ready() themselves: a call that fans out cannot skip it;
// one that may leave without touching a shard, or walks the shards by itself, says ready() where its checks end.
// The column calls (delete, groups, attributes) deliver nothing: they hold the frame for the lock alone.
struct ShardedCall {
    mi_knn_sharded* t;
    std::unique_lock<std::mutex> lock;
    uint32_t n;
    ShardRoute ids;
    bool delivered = false;
    explicit ShardedCall(mi_knn_sharded* table, const uint64_t* list = nullptr, uint64_t n_list = 0)
        : t(table), lock(locked(table)), n(table->n()) {
        route(list, n_list);
    }
    ShardedCall(const ShardedCall&) = delete;
    // (for a call whose other checks come in front of the list's)
    void route(const uint64_t* list, uint64_t n_list) { ids = route_ids(t, list, n_list, NULL_IS_NO_LIST); }
    void ready() {
        if (!delivered) sharded_deliver_all(t);
        delivered = true;
    }
    // f(si, shard) for every shard
    template <class F>
    void for_each_shard(F&& f) {
        ready();
        fan_out(n, [&](size_t si) { f((uint32_t)si, t->shard[si]); },
                [](size_t si, int code, const char* msg) { fail(code, "shard %u: %s", (uint32_t)si, msg); });
    }
    // f(row shard, column shard) for every shard pair of one round of between_schedule (join_between_host.h: the pairs of a
    // round share no shard)
    template <class F>
    void for_each_shard_pair(const std::vector<std::pair<uint32_t, uint32_t>>& round, F&& f) {
        ready();
        fan_out(round.size(), [&](size_t pi) { f(round[pi].first, round[pi].second); },
                [&](size_t pi, int code, const char* msg) { fail(code, "shards %u x %u: %s", round[pi].first, round[pi].second, msg); });
    }

private:
    static std::unique_lock<std::mutex> locked(mi_knn_sharded* table) {
        if (!table) fail(MI_ERR_INVALID, "null table handle");
        if (table->shard.empty()) fail(MI_ERR_INVALID, "a table without shards");
        return std::unique_lock<std::mutex>(table->mu);
    }
};

}  // namespace mi
#endif  // __HIPCC__
