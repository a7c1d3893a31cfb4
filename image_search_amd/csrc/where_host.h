// where_host.h — the host-only pieces of mi_knn_search_where and its kin (where.hip): the argument rules, the predicate on one
// row as the kernels evaluate it (where_row: what the host-side restatements are held against), the rule of "where_chunk" and
// the chunk count.  No HIP in here: tests/cpp/test_where_host.cpp runs it under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mi355clip.h"

namespace mi {

constexpr uint32_t WHERE_K_MAX = 4096;          // the filtered search's limit: the search behind the predicate is that call's
constexpr uint32_t WHERE_CHUNK_DEFAULT = 4096;  // rows one workgroup of the two predicate passes owns (option "where_chunk")
constexpr uint32_t WHERE_CHUNK_MAX = 1u << 16;         // 1024 tiles: the emit pass keeps one ballot per tile in LDS (8 KiB)

// MI_OK, or the error the contract names with *why set: the predicate's pointer, its flags (MI_ERR_INVALID)
inline int where_check_pred(const mi_knn_where* w, const char** why) {
    *why = "";
    if (!w) { *why = "where is null"; return MI_ERR_INVALID; }
    if (w->flags & ~(uint32_t)MI_KNN_WHERE_GROUP) { *why = "unknown bits in where.flags"; return MI_ERR_INVALID; }
    return MI_OK;
}

// mi_knn_count_where / mi_knn_rows_where: handle, predicate, the count's pointer, an id array when cap says there is one
inline int where_check_rows_args(const void* t, const mi_knn_where* w, const void* ids, uint64_t cap, const void* count, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    const int bad = where_check_pred(w, why);
    if (bad != MI_OK) return bad;
    if (!count) { *why = "count is null"; return MI_ERR_INVALID; }
    if (cap && !ids) { *why = "ids is null"; return MI_ERR_INVALID; }
    return MI_OK;
}

// mi_knn_search_where, in the filtered search's order: handle, pointers (judged only when there is a query), the predicate,
// then k (0: MI_ERR_INVALID, above 4096: MI_ERR_UNSUPPORTED)
inline int where_check_search_args(const void* t, const void* q, uint32_t nq, uint32_t k, const mi_knn_where* w, const void* idx,
                                   const void* dist, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (nq && (!q || !idx || !dist)) { *why = "null query/result pointer"; return MI_ERR_INVALID; }
    const int bad = where_check_pred(w, why);
    if (bad != MI_OK) return bad;
    if (k == 0) { *why = "k must be >= 1"; return MI_ERR_INVALID; }
    if (k > WHERE_K_MAX) { *why = "k must be <= 4096"; return MI_ERR_UNSUPPORTED; }
    return MI_OK;
}

// mi_knn_set_attrs / mi_knn_get_attrs: a handle, and ids when there are rows to name
inline int where_check_attrs_args(const void* t, const void* ids, uint64_t n, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (n && !ids) { *why = "ids is null"; return MI_ERR_INVALID; }
    return MI_OK;
}

// The predicate on one LIVE row: what where_count_kernel and where_emit_kernel evaluate.  has_groups: the table has a group
// column (without one nothing matches under MI_KNN_WHERE_GROUP, whatever `group` says).
inline bool where_row(const mi_knn_where& w, uint64_t tags, int64_t stamp, bool has_groups, uint32_t group) {
    if ((tags & w.all_of) != w.all_of) return false;
    if (w.any_of != 0 && (tags & w.any_of) == 0) return false;
    if ((tags & w.none_of) != 0) return false;
    if (stamp < w.stamp_lo || stamp > w.stamp_hi) return false;
    if (w.flags & MI_KNN_WHERE_GROUP) return has_groups && group == w.group;
    return true;
}

// a predicate no row can meet, seen without looking at a row: an empty stamp range, a bit both required and forbidden, the
// group flag on a table without a group column
inline bool where_never(const mi_knn_where& w, bool has_groups) {
    if (w.stamp_lo > w.stamp_hi) return true;
    if (w.all_of & w.none_of) return true;
    return (w.flags & MI_KNN_WHERE_GROUP) && !has_groups;
}

// option "where_chunk": 0 = the default, otherwise a multiple of 64 up to 65536
inline bool where_chunk_ok(int v) { return v == 0 || (v > 0 && v % 64 == 0 && (uint32_t)v <= WHERE_CHUNK_MAX); }
inline uint32_t where_chunk_rows(int option) { return option > 0 ? (uint32_t)option : WHERE_CHUNK_DEFAULT; }
inline uint32_t where_chunks(uint64_t rows, uint32_t chunk) { return (uint32_t)((rows + chunk - 1) / chunk); }

}  // namespace mi
