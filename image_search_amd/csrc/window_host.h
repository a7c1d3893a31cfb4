// window_host.h — the host-only rules of the windowed pair calls (mi_knn_near_pairs_window, mi_knn_density_window,
// mi_knn_dbscan_window; window.hip): the stamp test, the gap between two blocks' stamp ranges, which tiles of a strip can
// hold a pair within the window, the column range a strip launches and the tiles it computes and skips.  The device code
// (window_kernels.h) includes this header for stamp_diff and range_gap, so host and device decide with the same lines.
// Nothing in here knows of HIP: tests/cpp/test_window_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifndef MI_HD
#ifdef __HIPCC__
#define MI_HD __host__ __device__
#else
#define MI_HD
#endif
#endif

namespace mi {

// |a - b| of two stamps, exactly: every pair of int64 values has a difference in [0, 2^64 - 1], and hi - lo taken in
// uint64 arithmetic is that difference (the subtraction wraps by 2^64 exactly when the signed one would overflow).
MI_HD inline uint64_t stamp_diff(int64_t a, int64_t b) {
    const int64_t hi = a < b ? b : a, lo = a < b ? a : b;
    return (uint64_t)hi - (uint64_t)lo;
}
// the stamp test: window 0 = equal stamps only, UINT64_MAX = every pair
MI_HD inline bool stamp_within(int64_t a, int64_t b, uint64_t window) { return stamp_diff(a, b) <= window; }

// The stamps of a block's rows lie in [lo, hi]; lo > hi: the block holds no live row (the range is empty).
struct StampRange { int64_t lo, hi; };
constexpr StampRange STAMP_RANGE_EMPTY = {INT64_MAX, INT64_MIN};
MI_HD inline bool range_is_empty(StampRange r) { return r.lo > r.hi; }
// The smallest |s - t| over s in a, t in b, both not empty: 0 when the ranges meet, else the distance between the nearer
// ends (exact, as stamp_diff).
MI_HD inline uint64_t range_gap(StampRange a, StampRange b) {
    if (a.hi < b.lo) return stamp_diff(b.lo, a.hi);
    if (b.hi < a.lo) return stamp_diff(a.lo, b.hi);
    return 0;
}
// Can a tile of the two blocks hold a pair that passes the stamp test?  No row, no pair; else every pair of the tile is at
// least the gap apart, and some pair of values of the two ranges is exactly the gap apart: the tile is skipped iff
// gap > window.  (A range may be wider than its live rows' stamps — deleted rows may be counted in: the gap only shrinks.)
MI_HD inline bool window_tile_live(StampRange a, StampRange b, uint64_t window) {
    return !range_is_empty(a) && !range_is_empty(b) && range_gap(a, b) <= window;
}

// The blocks of one table as a windowed pass sees them: the stamp ranges and, in pass 2 of the windowed DBSCAN, the activity
// bytes (density_host.h: bit 0 = some row has a neighbour, bit 1 = some row is a core; empty: pass 1, no such test).
struct WindowBlocks {
    std::vector<StampRange> range;
    std::vector<uint8_t> act;
    uint64_t window = 0;

    // tile (bi, bj) is computed iff neither test skips it
    bool computed(uint32_t bi, uint32_t bj) const {
        if (!window_tile_live(range[bi], range[bj], window)) return false;
        if (act.empty()) return true;
        const uint8_t fa = act[bi], fb = act[bj];
        return (fa & fb & 1u) && ((fa | fb) & 2u);
    }
};

// What one stage-1 launch of a self pass does with the tile rows [r0, r1) x tile columns [c0, c1), on or above the diagonal
// (tile row bi owns the columns max(c0, bi) .. c1 - 1).
struct WindowStrip {
    uint32_t lo = 0, hi = 0;               // the columns to launch: [lo, hi), the smallest range that holds every computed tile
    uint64_t computed = 0, skipped = 0;    // of the tiles of the ground; computed + skipped = the ground's triangle
    bool launches() const { return computed != 0; }   // no computed tile: nothing is launched
};
inline WindowStrip window_strip(const WindowBlocks& w, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
    WindowStrip s;
    uint32_t lo = c1, hi = c0;
    uint64_t all = 0;
    for (uint32_t bi = r0; bi < r1; ++bi) {
        const uint32_t first = std::max(c0, bi);
        if (first >= c1) continue;
        all += c1 - first;
        if (range_is_empty(w.range[bi])) continue;
        for (uint32_t bj = first; bj < c1; ++bj) {
            if (!w.computed(bi, bj)) continue;
            ++s.computed;
            lo = std::min(lo, bj);
            hi = std::max(hi, bj + 1);
        }
    }
    s.skipped = all - s.computed;
    if (s.computed) { s.lo = lo; s.hi = hi; }
    return s;
}

}  // namespace mi
