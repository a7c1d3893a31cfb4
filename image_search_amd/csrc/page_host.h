// page_host.h — the host-only pieces of mi_knn_search_page (page.hip): the argument rules, the search's key transform as the
// host needs it (the cursor and the bound are keys), the cursor -> first_key rule for a table, for a shard of a block-cyclic
// table and for the sharded call (on the id space of ids.h), the `hi` rule, the per-CU factor of "page_blocks", and the layout
// of the one record the device writes with how it (or "no candidate") reaches the caller's arrays.  No HIP in here:
// tests/cpp/test_page_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../include/mi355clip.h"
#include "ids.h"

namespace mi {

constexpr uint32_t PAGE_K_MAX = 4096;

// dist_to_u32 of knn_shared.h on the host: numeric order, -0 before +0, every NaN last and equal
inline uint32_t page_dist_key(float d) {
    uint32_t b;
    std::memcpy(&b, &d, sizeof b);
    if (d != d) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// MI_OK, or the error the contract names with *why set, in the contract's order: the candidates' pointer rule, the cursor,
// the bound (all MI_ERR_INVALID), then k (0: MI_ERR_INVALID, above 4096: MI_ERR_UNSUPPORTED).  What needs the table — the dim,
// "after_id is a row", "every id of among is a row" — is judged under the handle's lock (page_first_key, knn_filter_rows).
inline int page_check_args(const void* t, const float* q, uint32_t k, float after_dist, uint64_t after_id, float max_dist,
                           const void* among, uint64_t n_among, const void* idx, const void* dist, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (!q || !idx || !dist) { *why = "null query/result pointer"; return MI_ERR_INVALID; }
    if (!among && n_among != 0) { *why = "among is null"; return MI_ERR_INVALID; }
    if (after_id != MI_KNN_NO_ID && after_dist != after_dist) { *why = "after_dist is NaN"; return MI_ERR_INVALID; }
    if (max_dist != max_dist) { *why = "max_dist is NaN"; return MI_ERR_INVALID; }
    if (k == 0) { *why = "k must be >= 1"; return MI_ERR_INVALID; }
    if (k > PAGE_K_MAX) { *why = "k must be <= 4096"; return MI_ERR_UNSUPPORTED; }
    return MI_OK;
}

// The scan's lower end is INCLUSIVE: a candidate is past the cursor iff key >= first_key.  `below` = the table's local rows
// whose id is <= after_id: with the cursor's own row in the table that is its local row + 1, i.e. first_key = cursor key + 1
// (the carry into the distance word at row 0xFFFFFFFF is the right answer: nothing of that distance is left).  A shard that
// does not hold the cursor's row places the row part freely the same way.  The distance word is built from after_dist's bits
// as given (-0 and +0 differ); after_dist is not NaN, so the sum cannot wrap.
inline uint64_t page_first_key_at(float after_dist, uint64_t below) { return ((uint64_t)page_dist_key(after_dist) << 32) + below; }

// one table of `rows` rows (ids.h): false when after_id names no row of it (MI_ERR_INVALID); no cursor (MI_KNN_NO_ID): 0,
// after_dist ignored.  A shard under the sharded call: page_first_key_at(after_dist, cyclic_rows_of(.., after_id + 1)).
inline bool page_first_key(const IdMap& m, uint64_t rows, float after_dist, uint64_t after_id, uint64_t* first_key) {
    *first_key = 0;
    if (after_id == MI_KNN_NO_ID) return true;
    uint64_t local = 0;
    if (!local_of_id(m, rows, after_id, &local)) return false;
    *first_key = page_first_key_at(after_dist, local + 1);
    return true;
}

// the upper end, inclusive, on the key order: every row part of the bound's distance
inline uint64_t page_hi(float max_dist) { return ((uint64_t)page_dist_key(max_dist) << 32) | 0xFFFFFFFFull; }

// the scan's workgroups with "page_blocks" = 0: the single pass's grid, four per CU (scan_grid of scan_call.h)
constexpr uint32_t PAGE_BLOCKS_PER_CU = 4;

// The record: idx [k] u64 | counts [4] u64 = {before, window, beyond, nan} | dist [k] f32
struct PageRecord {
    size_t idx, counts, dist, bytes;
};
inline PageRecord page_record(uint32_t k) {
    PageRecord r;
    r.idx = 0;
    r.counts = (size_t)k * sizeof(uint64_t);
    r.dist = r.counts + 4 * sizeof(uint64_t);
    r.bytes = r.dist + (size_t)k * sizeof(float);
    return r;
}
inline void page_unpack(const unsigned char* rec, uint32_t k, uint64_t* idx, float* dist, uint64_t* counts /* nullable */) {
    const PageRecord r = page_record(k);
    std::memcpy(idx, rec + r.idx, (size_t)k * sizeof(uint64_t));
    std::memcpy(dist, rec + r.dist, (size_t)k * sizeof(float));
    if (counts) std::memcpy(counts, rec + r.counts, 4 * sizeof(uint64_t));
}

// no candidate at all: all padding, every count 0
inline void page_pad(uint32_t k, uint64_t* idx, float* dist, uint64_t* counts /* nullable */) {
    for (uint32_t j = 0; j < k; ++j) {
        idx[j] = MI_KNN_NO_ID;
        dist[j] = std::numeric_limits<float>::infinity();
    }
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
}

}  // namespace mi
