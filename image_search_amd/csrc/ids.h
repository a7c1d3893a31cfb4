// ids.h — the id space of a table, in one place: local row <-> id for a plain table and for a shard of a block-cyclic table, and
// the placement arithmetic of the block-cyclic table itself.  The kernels turn local rows into ids with id_of_local (IdMap is a
// kernel argument: its fields keep their order and types); the host checks ids, builds cursors and routes rows with the rest.
// The functions the kernels share with the host are marked for both sides when a HIP compiler reads this file; nothing else in
// here knows of HIP: tests/cpp/test_ids_host.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define MI_IDS_HD __host__ __device__
#else
#define MI_IDS_HD
#endif

namespace mi {

// Row ids of a table.  Plain: id = base + local ordinal.  Block-cyclic (a shard of mi_knn_sharded: global row r lives in
// block r / B, blocks are dealt round-robin to the n shards): id = base + ((local / B) * n + rank) * B + local % B —
// monotone in the local ordinal, so "(distance asc, local asc)" inside a shard IS "(distance asc, id asc)".
struct IdMap { uint64_t base; uint32_t block, n, rank; };
MI_IDS_HD inline uint64_t id_of_local(const IdMap& m, uint64_t local) {
    if (m.n <= 1 || m.block == 0) return m.base + local;
    return m.base + ((local / m.block) * m.n + m.rank) * m.block + local % m.block;
}

// the inverse, for a table of `rows` rows: id -> local row, deleted or not; false if the table holds no such row
inline bool local_of_id(const IdMap& m, uint64_t rows, uint64_t id, uint64_t* local) {
    if (id < m.base) return false;
    const uint64_t off = id - m.base;
    uint64_t l = off;
    if (m.n > 1 && m.block) {
        const uint64_t b = off / m.block;
        if (b % m.n != m.rank) return false;
        l = (b / m.n) * m.block + off % m.block;
    }
    if (l >= rows) return false;
    *local = l;
    return true;
}

// The block-cyclic table of n shards (mi_knn_sharded_place): global row r lives in block r / block, block b on shard b % n at
// local block b / n.
inline void cyclic_place(uint32_t block, uint32_t n, uint64_t r, uint32_t* s, uint64_t* local) {
    const uint64_t blk = r / block;
    *s = (uint32_t)(blk % n);
    *local = (blk / n) * block + r % block;
}
// (and back: id_of_local of IdMap{0, block, n, s}).  The rows shard s holds of a table of `total` rows.  A shard's local rows ascend with their global ids, so these are its FIRST
// rows: with total = r + 1, the local rows of s whose global row is <= r, whether s holds r or not (what a cursor needs).
inline uint64_t cyclic_rows_of(uint32_t block, uint32_t n, uint32_t s, uint64_t total) {
    const uint64_t full = total / block, rem = total % block;
    return (full / n + (s < full % n ? 1 : 0)) * block + (s == full % n ? rem : 0);
}

}  // namespace mi
