// summary_sharded_host.h — the host-only rules of mi_knn_sharded_summarize (summary_sharded.hip): how the caller's labels
// are dealt to the shards, how a shard's per-group slots (summary_host.h) turn from local rows to global ids and how the
// slots of two shards become one, and the bytes that cross between shards.  The two word rules are marked for both sides when
// a HIP compiler reads this file (summary_sharded_kernels.h applies them, one thread per group); nothing else in here knows of
// HIP: tests/cpp/test_summary_sharded_host.cpp runs it under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ids.h"
#include "summary_host.h"

namespace mi {

// ---- labels by global row -> a shard's local rows ---------------------------------------------------------------------------
// out[r] = labels[id_of_local(map, r)] for the n local rows of one shard: the inverse of scatter_to_global
// (density_sharded_host.h).  A shard of a sharded table has base 0: its ids are the table's global rows.
inline void summary_deal_labels(const IdMap& map, const uint32_t* labels, uint64_t n, uint32_t* out) {
    for (uint64_t r = 0; r < n; ++r) out[r] = labels[id_of_local(map, r)];
}

// ---- a shard's slots: local rows -> global ids ------------------------------------------------------------------------------
// Inside one shard local rows ascend with their global ids (ids.h), so the shard's own minimum and maximum already chose the
// member with the lowest id among equal keys: only the row in the low half of the word changes.  Across shards the local
// order says nothing (local row 0 of shard 1 lies behind a whole block of shard 0): the words are compared after this step
// alone.  A word that still holds its start value names no row and stays.  Ids are < 2^32 under the call's row limit.
MI_IDS_HD inline uint64_t summary_globalize_min(uint64_t w, const IdMap& map) {
    if (w == SUMMARY_MIN_INIT) return w;
    return (w & 0xFFFFFFFF00000000ull) | (uint32_t)id_of_local(map, (uint32_t)w);
}
MI_IDS_HD inline uint64_t summary_globalize_max(uint64_t w, const IdMap& map) {
    if (w == SUMMARY_MAX_INIT) return w;
    return (w & 0xFFFFFFFF00000000ull) | (uint32_t)~(uint32_t)id_of_local(map, (uint32_t)~(uint32_t)w);
}
// slots [4][C] of one shard, in place
inline void summary_globalize_slots(uint64_t* slots, uint32_t C, const IdMap& map) {
    for (uint32_t c = 0; c < C; ++c) {
        slots[c] = summary_globalize_min(slots[c], map);
        slots[(size_t)C + c] = summary_globalize_max(slots[(size_t)C + c], map);
    }
}

// ---- the slots of two shards -> one -----------------------------------------------------------------------------------------
// plane 0 the smaller word, plane 1 the larger, planes 2 and 3 added: integer operations, so the shards may arrive in any
// order.  Both sides hold global ids.
inline void summary_merge_slots(uint64_t* dst, const uint64_t* src, uint32_t C) {
    for (uint32_t c = 0; c < C; ++c) {
        if (src[c] < dst[c]) dst[c] = src[c];
        if (src[(size_t)C + c] > dst[(size_t)C + c]) dst[(size_t)C + c] = src[(size_t)C + c];
        dst[(size_t)2 * C + c] += src[(size_t)2 * C + c];
        dst[(size_t)3 * C + c] += src[(size_t)3 * C + c];
    }
}

// ---- what crosses between shards ----------------------------------------------------------------------------------------------
// sums (8 bytes per component), sizes (4 per group) and slots (32 per group) inward from every shard but the first, the
// centroids outward to the same shards
inline uint64_t summary_sharded_exchange_bytes(uint32_t S, uint32_t C, uint32_t dim) {
    if (S == 0) return 0;
    return (uint64_t)(S - 1) * C * (8ull * dim + 4 + 32) + (uint64_t)(S - 1) * 4ull * C * dim;
}

}  // namespace mi
