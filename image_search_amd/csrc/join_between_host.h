// join_between_host.h — the host-only rules of the join of two row sets (join_between.hip: mi_knn_near_pairs_between,
// mi_knn_sharded_near_pairs, mi_index_matches): the argument checks, the column chunks of a staged operand and the strips of
// tile rows, the two rectangles of tiles a (fn_a, fn_b) pair of bounds leaves to launch, a shard's local first_new, and the
// round-robin schedule of the shard pairs.  Nothing in here knows of HIP: tests/cpp/test_join_between_host.cpp runs it under
// the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/mi355clip.h"
#include "ids.h"

namespace mi {

constexpr uint32_t BETWEEN_TILE = 128;                       // rows of a stage-1 tile, both ways (tile128.h: TILE)
constexpr uint64_t BETWEEN_STAGE_BYTES = 256ull << 20;       // the fp32 rows of one staged column chunk fit this

// ---- the argument rules: MI_OK, or MI_ERR_INVALID with *why set; judged before a handle is followed -----------------------
inline int join_check_out(float max_dist, const void* a, const void* b, const void* dist, uint64_t cap, const void* count, const char** why) {
    if (!(max_dist >= 0.0f)) { *why = "max_dist must be a number >= 0"; return MI_ERR_INVALID; }
    if (!count) { *why = "count is null"; return MI_ERR_INVALID; }
    if (cap && (!a || !b || !dist)) { *why = "a, b or dist is null with cap > 0"; return MI_ERR_INVALID; }
    return MI_OK;
}
inline int between_check_args(const void* t, const void* other, float max_dist, const void* a, const void* b, const void* dist,
                              uint64_t cap, const void* count, const char** why) {
    *why = "";
    if (!t || !other) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (t == other) { *why = "the two tables are the same handle (mi_knn_near_pairs joins a table with itself)"; return MI_ERR_INVALID; }
    return join_check_out(max_dist, a, b, dist, cap, count, why);
}
inline int sharded_join_check_args(const void* t, float max_dist, const void* a, const void* b, const void* dist, uint64_t cap,
                                   const void* count, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    return join_check_out(max_dist, a, b, dist, cap, count, why);
}

// ---- chunks of the column operand and strips of tile rows ------------------------------------------------------------
// rows of one staged chunk: `forced` (option "join_stage_rows", rounded up to whole tiles) or what the budget holds, whole
// tiles, at least one
inline uint32_t between_chunk_rows(uint32_t dim, uint32_t forced, uint64_t budget = BETWEEN_STAGE_BYTES) {
    uint64_t rows = forced ? forced : budget / ((uint64_t)std::max(dim, 1u) * sizeof(float));
    rows = (forced ? (rows + BETWEEN_TILE - 1) : rows) / BETWEEN_TILE * BETWEEN_TILE;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(rows, BETWEEN_TILE), 1u << 30);
}
inline uint32_t between_n_chunks(uint64_t n_b, uint32_t chunk_rows) { return (uint32_t)((n_b + chunk_rows - 1) / chunk_rows); }
// chunk i of n_b rows: [c0, c1); the chunks tile [0, n_b) in order, every one but the last holds chunk_rows
inline void between_chunk(uint64_t n_b, uint32_t chunk_rows, uint32_t i, uint64_t* c0, uint64_t* c1) {
    *c0 = std::min<uint64_t>(n_b, (uint64_t)i * chunk_rows);
    *c1 = std::min<uint64_t>(n_b, *c0 + chunk_rows);
}
// a bound on B's local rows as a bound on the rows of chunk [c0, c1)
inline uint32_t between_chunk_bound(uint64_t fn_b, uint64_t c0, uint64_t c1) { return (uint32_t)(std::min(std::max(fn_b, c0), c1) - c0); }

// tile rows per stage-1 launch over n_cols column tiles (the self-join's rule): enough tiles to fill the device a few
// times over, few enough that an ordinary corpus never meets the candidate buffer's end
inline uint32_t between_strip(uint32_t n_cols) { return std::max<uint32_t>(1u, std::min<uint32_t>(256u, (1u << 18) / std::max(n_cols, 1u))); }

// The tile rows [r0, r1) against the tile columns [c0, c1), in strips of between_strip(c1 - c0) tile rows: the one strip walk
// of the self-join, the join of two row sets and the density passes.  rect(br0, br1, c0, c1, &overflowed) runs one strip
// (rect_stages with the caller's two stages) and reports whether its candidates overflowed the buffer: the strips after it
// are half as tall, never below one tile row.  stop() ends the walk between strips.
template <class Rect, class Stop>
void tile_strips(uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, Rect&& rect, Stop&& stop) {
    if (c0 >= c1) return;
    uint32_t strip = between_strip(c1 - c0);
    for (uint32_t br = r0; br < r1 && !stop();) {
        const uint32_t end = std::min(r1, br + strip);
        bool overflowed = false;
        rect(br, end, c0, c1, &overflowed);
        if (overflowed) strip = std::max(1u, strip / 2);
        br = end;
    }
}

// ---- the tiles to launch -------------------------------------------------------------------------------------------------
// Element (ra, cb) of n_a x n_b rows qualifies iff ra >= fn_a or cb >= fn_b (fn_a <= n_a, fn_b <= n_b; 0, 0: everything).
// A tile is launched iff it holds a qualifying element: tile row bi has one by its rows iff bi >= ta, tile column bj by its
// columns iff bj >= tb, with ta / tb the tile of the first row / column at or above the bound (none: the tile count).  That
// is the rectangle [ta, nba) x [0, nbb) and, below it, [0, ta) x [tb, nbb).  Returns how many of the two are not empty.
struct TileRect { uint32_t r0, r1, c0, c1; };
inline uint32_t between_tiles_of(uint64_t n) { return (uint32_t)((n + BETWEEN_TILE - 1) / BETWEEN_TILE); }
inline uint32_t between_rects(uint64_t n_a, uint64_t n_b, uint64_t fn_a, uint64_t fn_b, TileRect out[2]) {
    const uint32_t nba = between_tiles_of(n_a), nbb = between_tiles_of(n_b);
    const uint32_t ta = fn_a >= n_a ? nba : (uint32_t)(fn_a / BETWEEN_TILE), tb = fn_b >= n_b ? nbb : (uint32_t)(fn_b / BETWEEN_TILE);
    uint32_t n = 0;
    if (nbb == 0 || nba == 0) return 0;
    if (ta < nba) out[n++] = TileRect{ta, nba, 0, nbb};
    if (ta > 0 && tb < nbb) out[n++] = TileRect{0, ta, tb, nbb};
    return n;
}

// ---- the sharded join -----------------------------------------------------------------------------------------------------
// first_new (a global id, 0 = everything, up to one past the last row) as a bound on shard s's local rows: the number of its
// rows whose global id is below first_new (a shard's local rows ascend with their ids)
inline uint64_t shard_first_new(uint32_t block, uint32_t n, uint32_t s, uint64_t first_new) {
    return first_new == 0 ? 0 : cyclic_rows_of(block, n, s, first_new);
}

// The S (S - 1) / 2 shard pairs in rounds (the circle method): every pair occurs once, a shard is in at most one pair of a
// round, so the pairs of a round run side by side on different devices.  first = the row side (where the work runs), second =
// the column side: of shards x < y, x when x + y is odd and y otherwise, so that every shard is the row side of about half
// of its pairs and the work spreads over the devices.
typedef std::pair<uint32_t, uint32_t> ShardPair;
inline std::vector<std::vector<ShardPair>> between_schedule(uint32_t S) {
    std::vector<std::vector<ShardPair>> rounds;
    if (S < 2) return rounds;
    const uint32_t m = S + (S & 1u);   // an odd count gets a bye
    std::vector<uint32_t> ring(m);
    for (uint32_t i = 0; i < m; ++i) ring[i] = i;
    for (uint32_t r = 0; r + 1 < m; ++r) {
        std::vector<ShardPair> round;
        for (uint32_t i = 0; i < m / 2; ++i) {
            const uint32_t x = std::min(ring[i], ring[m - 1 - i]), y = std::max(ring[i], ring[m - 1 - i]);
            if (y >= S) continue;
            round.push_back(((x + y) & 1u) ? ShardPair(x, y) : ShardPair(y, x));
        }
        rounds.push_back(round);
        std::rotate(ring.begin() + 1, ring.end() - 1, ring.end());   // the first stays, the others move one place on
    }
    return rounds;
}

}  // namespace mi
