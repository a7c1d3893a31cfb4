// The host-only pieces of the windowed pair calls (image_search_amd/csrc/window_host.h) as a stand-alone program: the exact
// stamp difference and the gap between two blocks' ranges on the extremes of int64, empty ranges, the columns a strip
// launches (banded, full, all skipped) and the computed / skipped counts against a brute-force walk over random ranges.
// Built with -fsanitize=address,undefined (tests/test_window_host.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../image_search_amd/csrc/window_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void stamps() {
    EXPECT(stamp_diff(5, 5) == 0 && stamp_within(5, 5, 0) && !stamp_within(5, 6, 0));
    EXPECT(stamp_diff(10, 110) == 100 && stamp_within(10, 110, 100) && stamp_within(110, 10, 100));
    EXPECT(stamp_diff(10, 111) == 101 && !stamp_within(10, 111, 100) && !stamp_within(111, 10, 100));
    EXPECT(stamp_diff(INT64_MIN, INT64_MAX) == UINT64_MAX && stamp_diff(INT64_MAX, INT64_MIN) == UINT64_MAX);
    EXPECT(!stamp_within(INT64_MIN, INT64_MAX, UINT64_MAX - 1) && stamp_within(INT64_MIN, INT64_MAX, UINT64_MAX));
    EXPECT(stamp_diff(INT64_MIN, 0) == (1ull << 63) && !stamp_within(INT64_MIN, 0, (1ull << 63) - 1) && stamp_within(0, INT64_MIN, 1ull << 63));
    EXPECT(stamp_diff(INT64_MAX, 0) == (1ull << 63) - 1);
    EXPECT(stamp_diff(-1, 1) == 2 && !stamp_within(-1, 1, 1) && stamp_within(1, -1, 2));
    EXPECT(stamp_diff(INT64_MIN, INT64_MIN) == 0 && stamp_diff(INT64_MAX, INT64_MAX) == 0 && stamp_diff(INT64_MIN, INT64_MIN + 1) == 1);
}

static void gaps() {
    const StampRange lowest = {INT64_MIN, INT64_MIN}, highest = {INT64_MAX, INT64_MAX}, all = {INT64_MIN, INT64_MAX}, zero = {0, 0};
    EXPECT(range_gap(lowest, highest) == UINT64_MAX && range_gap(highest, lowest) == UINT64_MAX);
    EXPECT(!window_tile_live(lowest, highest, UINT64_MAX - 1) && window_tile_live(lowest, highest, UINT64_MAX));
    EXPECT(range_gap(all, zero) == 0 && range_gap(zero, all) == 0 && range_gap(all, all) == 0 && window_tile_live(all, lowest, 0));
    EXPECT(range_gap(lowest, zero) == (1ull << 63) && range_gap(zero, highest) == (1ull << 63) - 1);
    const StampRange a = {10, 20}, b = {21, 30}, c = {20, 25}, d = {-5, 9};
    EXPECT(range_gap(a, b) == 1 && range_gap(b, a) == 1 && range_gap(a, c) == 0 && range_gap(c, a) == 0 && range_gap(a, d) == 1);
    EXPECT(!window_tile_live(a, b, 0) && window_tile_live(a, b, 1) && window_tile_live(a, c, 0) && window_tile_live(a, a, 0));
    // an empty range skips against everything, also against itself and at the widest window
    EXPECT(range_is_empty(STAMP_RANGE_EMPTY) && !range_is_empty(zero) && !range_is_empty(all));
    EXPECT(!window_tile_live(STAMP_RANGE_EMPTY, all, UINT64_MAX) && !window_tile_live(all, STAMP_RANGE_EMPTY, UINT64_MAX));
    EXPECT(!window_tile_live(STAMP_RANGE_EMPTY, STAMP_RANGE_EMPTY, UINT64_MAX));
}

static uint64_t triangle(uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
    uint64_t n = 0;
    for (uint32_t bi = r0; bi < r1; ++bi)
        for (uint32_t bj = c0 > bi ? c0 : bi; bj < c1; ++bj) ++n;
    return n;
}

static void strips() {
    // ascending stamps, block b holds [100 b, 100 b + 99]: at window 150 tile (bi, bj) survives iff bj - bi <= 2 (gap 1, 101, 201)
    WindowBlocks w;
    for (int b = 0; b < 10; ++b) w.range.push_back(StampRange{100 * b, 100 * b + 99});
    w.window = 150;
    WindowStrip s = window_strip(w, 2, 4, 0, 10);       // rows 2, 3 from the diagonal: columns 2..4 and 3..5
    EXPECT(s.launches() && s.lo == 2 && s.hi == 6 && s.computed == 6 && s.skipped == triangle(2, 4, 0, 10) - 6);
    s = window_strip(w, 2, 4, 5, 10);                   // a column half of that strip: only (3, 5)
    EXPECT(s.launches() && s.lo == 5 && s.hi == 6 && s.computed == 1 && s.skipped == 9);
    s = window_strip(w, 2, 4, 6, 10);                   // all skipped: nothing to launch
    EXPECT(!s.launches() && s.computed == 0 && s.skipped == 8);
    s = window_strip(w, 8, 10, 0, 10);                  // the ragged end of the triangle
    EXPECT(s.lo == 8 && s.hi == 10 && s.computed == 3 && s.skipped == 0);
    w.window = UINT64_MAX;                              // a full strip
    s = window_strip(w, 0, 10, 0, 10);
    EXPECT(s.lo == 0 && s.hi == 10 && s.computed == 55 && s.skipped == 0);
    w.window = 0;                                       // ranges of different blocks never meet: the diagonal alone
    s = window_strip(w, 0, 10, 0, 10);
    EXPECT(s.lo == 0 && s.hi == 10 && s.computed == 10 && s.skipped == 45);
    s = window_strip(w, 4, 4, 0, 10);                   // no rows, and columns wholly below the diagonal
    EXPECT(!s.launches() && s.computed == 0 && s.skipped == 0);
    s = window_strip(w, 6, 8, 0, 5);
    EXPECT(!s.launches() && s.computed == 0 && s.skipped == 0);
    // an empty block in the middle of a strip is skipped as a row and as a column
    w.window = UINT64_MAX;
    w.range[3] = STAMP_RANGE_EMPTY;
    s = window_strip(w, 2, 5, 0, 10);
    EXPECT(s.lo == 2 && s.hi == 10 && s.computed == (8 - 1) + (6 - 0) && s.skipped == 1 + 7);
    // pass 2: the activity bytes take tiles away on top (both blocks bit 0, one of them bit 1)
    w.range[3] = StampRange{300, 399};
    w.window = 150;
    w.act.assign(10, 1);
    w.act[4] = 3;
    s = window_strip(w, 2, 4, 0, 10);                   // of the six banded tiles only those with block 4: (2, 4), (3, 4)
    EXPECT(s.lo == 4 && s.hi == 5 && s.computed == 2 && s.skipped == triangle(2, 4, 0, 10) - 2);
    w.act[4] = 1;
    s = window_strip(w, 2, 4, 0, 10);
    EXPECT(!s.launches() && s.skipped == triangle(2, 4, 0, 10));
}

static void random_ranges() {
    for (int round = 0; round < 300; ++round) {
        const uint32_t nb = 1 + (uint32_t)(rnd() % 24);
        WindowBlocks w;
        const int kind = round % 3;                     // small stamps, the whole int64 range, ascending
        for (uint32_t b = 0; b < nb; ++b) {
            int64_t x, y;
            if (kind == 0) { x = (int64_t)(rnd() % 2000) - 1000; y = (int64_t)(rnd() % 2000) - 1000; }
            else if (kind == 1) { x = (int64_t)rnd(); y = (int64_t)rnd(); }
            else { x = (int64_t)b * 50 + (int64_t)(rnd() % 60); y = x + (int64_t)(rnd() % 60); }
            w.range.push_back(rnd() % 7 == 0 ? STAMP_RANGE_EMPTY : StampRange{x < y ? x : y, x < y ? y : x});
        }
        w.window = kind == 1 ? rnd() : rnd() % 300;
        if (round % 5 == 0) w.window = UINT64_MAX;
        if (round % 2) { for (uint32_t b = 0; b < nb; ++b) w.act.push_back((uint8_t)(rnd() % 4)); }
        const uint32_t r0 = (uint32_t)(rnd() % nb), r1 = r0 + (uint32_t)(rnd() % (nb - r0 + 1));
        const uint32_t c0 = (uint32_t)(rnd() % nb), c1 = c0 + (uint32_t)(rnd() % (nb - c0 + 1));
        const WindowStrip s = window_strip(w, r0, r1, c0, c1);
        uint64_t computed = 0;
        uint32_t lo = c1, hi = c0;
        for (uint32_t bi = r0; bi < r1; ++bi)
            for (uint32_t bj = c0 > bi ? c0 : bi; bj < c1; ++bj) {
                const StampRange a = w.range[bi], b = w.range[bj];
                bool live = a.lo <= a.hi && b.lo <= b.hi;
                if (live) {   // the gap in 128-bit arithmetic
                    const __int128 g1 = (__int128)b.lo - a.hi, g2 = (__int128)a.lo - b.hi, g = g1 > g2 ? g1 : g2;
                    live = (g > 0 ? (unsigned __int128)g : 0) <= (unsigned __int128)w.window;
                }
                if (live && !w.act.empty()) live = (w.act[bi] & w.act[bj] & 1) && ((w.act[bi] | w.act[bj]) & 2);
                EXPECT(live == w.computed(bi, bj));
                if (live) { ++computed; lo = bj < lo ? bj : lo; hi = bj + 1 > hi ? bj + 1 : hi; }
            }
        EXPECT(s.computed == computed && s.computed + s.skipped == triangle(r0, r1, c0, c1));
        EXPECT(s.launches() == (computed != 0));
        if (computed) EXPECT(s.lo == lo && s.hi == hi && c0 <= s.lo && s.hi <= c1);
    }
}

int main() {
    stamps();
    gaps();
    strips();
    random_ranges();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
