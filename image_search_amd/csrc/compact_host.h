// compact_host.h — the host-only rules of mi_knn_compact (compact.hip): where every surviving row comes from, the old-to-new id
// map and the plan of chunks with its straight / staged decision (the columns' host copies: columns_host.h).  No HIP in
// here: tests/cpp/test_compact_host.cpp compiles this header alone and runs it under the sanitizers.
//
// `dead` is always the table's list of deleted local rows: ascending, once each, every one below `rows`.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "columns_host.h"   // compact_column: the same for a column's host copy

namespace mi {

constexpr uint64_t COMPACT_NO_ID = ~0ull;             // MI_KNN_NO_ID
constexpr uint64_t COMPACT_STAGE_BYTES = 64ull << 20;  // the staging buffer of the default chunk: 64 MiB, whatever the table's size
constexpr uint64_t COMPACT_MAX_PIECES = 1ull << 31;    // 16-byte pieces one launch of the move kernel indexes (32-bit arithmetic)

// The source row of destination row j (j < rows - dead.size()): the j-th live row.  It is j + c, c = the deleted rows below
// it = the first c with dead[c] - c > j (dead[c] - c, the live rows below dead[c], never decreases).  compact_src_kernel
// is the same search on the device.
inline uint64_t compact_src(const uint32_t* dead, size_t n_dead, uint64_t j) {
    size_t lo = 0, hi = n_dead;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)dead[mid] - mid > j) hi = mid;
        else lo = mid + 1;
    }
    return j + lo;
}
inline uint64_t compact_src(const std::vector<uint32_t>& dead, uint64_t j) { return compact_src(dead.data(), dead.size(), j); }

// new_ids[o] for every old local row o < rows: base + (o - the deleted rows below o), COMPACT_NO_ID for a deleted row
inline void compact_map(const std::vector<uint32_t>& dead, uint64_t rows, uint64_t base, uint64_t* new_ids) {
    size_t c = 0;
    for (uint64_t o = 0; o < rows; ++o) {
        if (c < dead.size() && dead[c] == o) { new_ids[o] = COMPACT_NO_ID; ++c; }
        else new_ids[o] = base + (o - c);
    }
}

// destination rows of one chunk: option "compact_chunk_rows" (0 = what COMPACT_STAGE_BYTES holds of rows of this dim), never
// more than one launch's 32-bit piece index reaches
inline uint64_t compact_chunk_rows(int option, uint32_t dim) {
    const uint64_t row_bytes = (uint64_t)dim * 4, pieces = row_bytes / 16;
    const uint64_t want = option > 0 ? (uint64_t)option : std::max<uint64_t>(1, COMPACT_STAGE_BYTES / row_bytes);
    return std::max<uint64_t>(1, std::min(want, COMPACT_MAX_PIECES / std::max<uint64_t>(pieces, 1)));
}

// Destination rows [j0, j1).  straight: its first source row is >= j1, so (sources ascend) no row it writes is a row it or a
// later chunk reads, and it is gathered into place; otherwise it goes through the staging buffer.
struct CompactChunk {
    uint64_t j0, j1;
    bool staged;
};
// first = the first deleted row: rows below it stay where they are; live = rows - deleted = the rows afterwards; the chunks
// tile [first, live) in ascending order
struct CompactPlan {
    uint64_t first = 0, live = 0, n_straight = 0, n_staged = 0, stage_rows = 0;
    std::vector<CompactChunk> chunks;
};
inline CompactPlan compact_plan(const std::vector<uint32_t>& dead, uint64_t rows, uint64_t chunk_rows) {
    CompactPlan p;
    p.live = rows - dead.size();
    p.first = dead.empty() ? rows : dead.front();   // <= live: the deleted rows all lie in [first, rows)
    chunk_rows = std::max<uint64_t>(chunk_rows, 1);
    for (uint64_t j0 = p.first; j0 < p.live;) {
        const uint64_t j1 = j0 + std::min(chunk_rows, p.live - j0);
        const bool staged = compact_src(dead, j0) < j1;
        p.chunks.push_back(CompactChunk{j0, j1, staged});
        if (staged) { ++p.n_staged; p.stage_rows = std::max(p.stage_rows, j1 - j0); }
        else ++p.n_straight;
        j0 = j1;
    }
    return p;
}

}  // namespace mi
