// ordered_host.h — the host-only pieces of mi_knn_search_ordered and mi_knn_stamp_histogram (ordered.hip): the argument rules,
// the order key of a stamp, the cursor as the kernels compare it (for a table, for a shard of a block-cyclic table and for the
// sharded call), the rule of the histogram's edges, the layout of the one record the device writes with how it (or "no
// candidate") reaches the caller's arrays, and the host merge of the shards' lists.  The two functions the kernels share with the
// host (ordered_okey, ordered_past) are marked for both sides when a HIP compiler reads this file; nothing else in here knows
// of HIP: tests/cpp/test_ordered_host.cpp runs it under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mi355clip.h"
#include "page_host.h"
#include "where_host.h"

#ifdef __HIPCC__
#define MI_ORDERED_HD __host__ __device__
#else
#define MI_ORDERED_HD
#endif

namespace mi {

constexpr uint32_t ORDERED_K_MAX = PAGE_K_MAX;
constexpr uint32_t ORDERED_EDGES_MAX = 4096;

// The order key of a stamp: unsigned order == signed order of the stamps, reversed under MI_KNN_ORDER_DESC.  The result order
// is (okey, id) ascending in both directions.
MI_ORDERED_HD inline uint64_t ordered_okey(int64_t stamp, bool desc) {
    const uint64_t k = (uint64_t)stamp ^ 0x8000000000000000ull;
    return desc ? ~k : k;
}
MI_ORDERED_HD inline int64_t ordered_stamp_of(uint64_t okey, bool desc) {
    return (int64_t)((desc ? ~okey : okey) ^ 0x8000000000000000ull);
}

// The cursor as the kernels take it.  Ids ascend with the local rows of a table (and of a shard), so "(okey, id) > (cursor okey,
// after_id)" is "okey > cursor okey, or okey == cursor okey and local row >= first_row" with first_row = the number of local
// rows whose id is <= after_id.  on == 0: no cursor, every row is past it.
struct OrderedCursor {
    uint64_t okey, first_row;
    uint32_t on, desc;
};
MI_ORDERED_HD inline bool ordered_past(const OrderedCursor& c, uint64_t okey, uint64_t row) {
    if (!c.on) return true;
    return okey > c.okey || (okey == c.okey && row >= c.first_row);
}

// MI_OK, or the error the contract names with *why set, in mi_knn_search_page's order: handle, pointers, the bound (NaN:
// MI_ERR_INVALID; a negative bound is a bound), the flags, the predicate when there is one (where_host.h), then k (0:
// MI_ERR_INVALID, above 4096: MI_ERR_UNSUPPORTED).  "after_id is a row" and the dim need the table: judged under its lock.
inline int ordered_check_args(const void* t, const float* q, uint32_t k, float max_dist, const mi_knn_where* w, uint32_t flags,
                              const void* idx, const void* dist, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!q || !idx || !dist) { *why = "null query/result pointer"; return MI_ERR_INVALID; }
    if (max_dist != max_dist) { *why = "max_dist is NaN"; return MI_ERR_INVALID; }
    if (flags & ~(uint32_t)(MI_KNN_ORDER_DESC | MI_KNN_ORDER_AFTER)) { *why = "unknown bits in flags"; return MI_ERR_INVALID; }
    if (w) {
        const int bad = where_check_pred(w, why);
        if (bad != MI_OK) return bad;
    }
    if (k == 0) { *why = "k must be >= 1"; return MI_ERR_INVALID; }
    if (k > ORDERED_K_MAX) { *why = "k must be <= 4096"; return MI_ERR_UNSUPPORTED; }
    return MI_OK;
}

// edges: strictly ascending, 1 <= n_edges <= 4096
inline bool ordered_edges_ok(const int64_t* edges, uint32_t n_edges, const char** why) {
    *why = "";
    if (!edges) { *why = "edges is null"; return false; }
    if (n_edges == 0 || n_edges > ORDERED_EDGES_MAX) { *why = "n_edges must be in [1, 4096]"; return false; }
    for (uint32_t i = 1; i < n_edges; ++i)
        if (!(edges[i - 1] < edges[i])) { *why = "edges must be strictly ascending"; return false; }
    return true;
}
inline int ordered_check_hist_args(const void* t, const float* q, float max_dist, const mi_knn_where* w, const int64_t* edges,
                                   uint32_t n_edges, const void* hist, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!q || !hist) { *why = "null query/result pointer"; return MI_ERR_INVALID; }
    if (max_dist != max_dist) { *why = "max_dist is NaN"; return MI_ERR_INVALID; }
    if (w) {
        const int bad = where_check_pred(w, why);
        if (bad != MI_OK) return bad;
    }
    return ordered_edges_ok(edges, n_edges, why) ? MI_OK : MI_ERR_INVALID;
}
// the bin of a stamp: how many edges are <= it (what the kernel's binary search returns)
inline uint32_t ordered_bin(const int64_t* edges, uint32_t n_edges, int64_t stamp) {
    uint32_t lo = 0, hi = n_edges;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (edges[mid] <= stamp) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one table of `rows` rows: false when MI_KNN_ORDER_AFTER is set and after_id names no row of it (deleted or not)
inline bool ordered_cursor(const IdMap& m, uint64_t rows, uint32_t flags, int64_t after_stamp, uint64_t after_id, OrderedCursor* c) {
    const bool desc = (flags & MI_KNN_ORDER_DESC) != 0;
    *c = OrderedCursor{0, 0, 0, desc ? 1u : 0u};
    if (!(flags & MI_KNN_ORDER_AFTER)) return true;
    uint64_t local = 0;
    if (!local_of_id(m, rows, after_id, &local)) return false;
    *c = OrderedCursor{ordered_okey(after_stamp, desc), local + 1, 1, desc ? 1u : 0u};
    return true;
}
// shard s of n (blocks of `block` rows dealt round-robin) under a cursor at global row after_row: the shard's rows at or below
// it are the rows it holds of a table of after_row + 1 rows, whether it holds the cursor's row or not
inline OrderedCursor ordered_cursor_shard(uint32_t block, uint32_t n, uint32_t s, uint32_t flags, int64_t after_stamp, uint64_t after_row) {
    const bool desc = (flags & MI_KNN_ORDER_DESC) != 0;
    if (!(flags & MI_KNN_ORDER_AFTER)) return OrderedCursor{0, 0, 0, desc ? 1u : 0u};
    return OrderedCursor{ordered_okey(after_stamp, desc), cyclic_rows_of(block, n, s, after_row + 1), 1, desc ? 1u : 0u};
}

// The record: idx [k] u64 | counts [4] u64 as the device leaves them = {before, within, beyond, nan} | stamps [k] i64 | dist [k] f32
struct OrderedRecord {
    size_t idx, counts, stamps, dist, bytes;
};
inline OrderedRecord ordered_record(uint32_t k) {
    OrderedRecord r;
    r.idx = 0;
    r.counts = (size_t)k * sizeof(uint64_t);
    r.stamps = r.counts + 4 * sizeof(uint64_t);
    r.dist = r.stamps + (size_t)k * sizeof(int64_t);
    r.bytes = r.dist + (size_t)k * sizeof(float);
    return r;
}
// counts as the caller gets them: {within, before, beyond, nan}
inline void ordered_unpack(const unsigned char* rec, uint32_t k, uint64_t* idx, float* dist, int64_t* stamps /* nullable */,
                           uint64_t* counts /* nullable */) {
    const OrderedRecord r = ordered_record(k);
    std::memcpy(idx, rec + r.idx, (size_t)k * sizeof(uint64_t));
    std::memcpy(dist, rec + r.dist, (size_t)k * sizeof(float));
    if (stamps) std::memcpy(stamps, rec + r.stamps, (size_t)k * sizeof(int64_t));
    if (counts) {
        uint64_t c[4];
        std::memcpy(c, rec + r.counts, sizeof c);
        counts[0] = c[1]; counts[1] = c[0]; counts[2] = c[2]; counts[3] = c[3];
    }
}
// no candidate at all: all padding, every count 0
inline void ordered_pad(uint32_t k, uint64_t* idx, float* dist, int64_t* stamps /* nullable */, uint64_t* counts /* nullable */) {
    for (uint32_t j = 0; j < k; ++j) {
        idx[j] = MI_KNN_NO_ID;
        dist[j] = std::numeric_limits<float>::infinity();
        if (stamps) stamps[j] = 0;
    }
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
}

// `lists` results of k slots each (ids global, every list in the result order, MI_KNN_NO_ID behind its hits) -> the first k of
// their union by (okey, id); padding behind.  stamps is required here (it is the order).
inline void ordered_merge(const uint64_t* idx, const float* dist, const int64_t* stamps, uint32_t lists, uint32_t k, bool desc,
                          uint64_t* o_idx, float* o_dist, int64_t* o_stamps /* nullable */) {
    std::vector<size_t> at(lists, 0);
    uint32_t slot = 0;
    for (; slot < k; ++slot) {
        uint32_t best = lists;
        for (uint32_t l = 0; l < lists; ++l) {
            if (at[l] >= k || idx[(size_t)l * k + at[l]] == MI_KNN_NO_ID) continue;
            if (best == lists) { best = l; continue; }
            const size_t a = (size_t)l * k + at[l], b = (size_t)best * k + at[best];
            const uint64_t ka = ordered_okey(stamps[a], desc), kb = ordered_okey(stamps[b], desc);
            if (ka < kb || (ka == kb && idx[a] < idx[b])) best = l;
        }
        if (best == lists) break;
        const size_t a = (size_t)best * k + at[best]++;
        o_idx[slot] = idx[a];
        o_dist[slot] = dist[a];
        if (o_stamps) o_stamps[slot] = stamps[a];
    }
    for (; slot < k; ++slot) {
        o_idx[slot] = MI_KNN_NO_ID;
        o_dist[slot] = std::numeric_limits<float>::infinity();
        if (o_stamps) o_stamps[slot] = 0;
    }
}

}  // namespace mi
