// The host-only pieces of the join of two row sets (image_search_amd/csrc/join_between_host.h) as a stand-alone program: the
// argument rules, the round-robin schedule of the shard pairs, the rectangles of tiles a pair of bounds leaves against a
// brute-force walk, a shard's local first_new against an enumeration of the ids, the column chunks, and the strip walk.  Built with
// -fsanitize=address,undefined (tests/test_join_between_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../image_search_amd/csrc/join_between_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void args() {
    const char* why = nullptr;
    int t = 0, u = 0, o = 0;
    EXPECT(between_check_args(&t, &u, 0.0f, &o, &o, &o, 4, &o, &why) == MI_OK && why[0] == '\0');
    EXPECT(between_check_args(&t, &u, INFINITY, nullptr, nullptr, nullptr, 0, &o, &why) == MI_OK);
    EXPECT(between_check_args(&t, &u, -0.0f, &o, &o, &o, 4, &o, &why) == MI_OK);   // -0 >= 0
    EXPECT(between_check_args(nullptr, &u, 0.1f, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(between_check_args(&t, nullptr, 0.1f, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(between_check_args(&t, &t, 0.1f, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID && std::strstr(why, "same"));
    EXPECT(between_check_args(&t, &u, NAN, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID && std::strstr(why, "max_dist"));
    EXPECT(between_check_args(&t, &u, -0.5f, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID);
    EXPECT(between_check_args(&t, &u, -INFINITY, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID);
    EXPECT(between_check_args(&t, &u, 0.1f, &o, &o, &o, 4, nullptr, &why) == MI_ERR_INVALID && std::strstr(why, "count"));
    EXPECT(between_check_args(&t, &u, 0.1f, nullptr, &o, &o, 4, &o, &why) == MI_ERR_INVALID);
    EXPECT(between_check_args(&t, &u, 0.1f, &o, &o, nullptr, 4, &o, &why) == MI_ERR_INVALID);
    EXPECT(sharded_join_check_args(&t, 0.1f, &o, &o, &o, 4, &o, &why) == MI_OK);
    EXPECT(sharded_join_check_args(nullptr, 0.1f, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(sharded_join_check_args(&t, NAN, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID);
    EXPECT(sharded_join_check_args(&t, -1.0f, &o, &o, &o, 4, &o, &why) == MI_ERR_INVALID);
    EXPECT(sharded_join_check_args(&t, 0.1f, &o, nullptr, &o, 4, &o, &why) == MI_ERR_INVALID);
}

// every shard pair exactly once, no shard twice in a round, the row side spread over the shards
static void schedule() {
    EXPECT(between_schedule(0).empty() && between_schedule(1).empty());
    for (uint32_t S = 1; S <= 9; ++S) {
        const auto rounds = between_schedule(S);
        std::set<std::pair<uint32_t, uint32_t>> seen;
        std::vector<uint32_t> row_side(S, 0);
        for (const auto& round : rounds) {
            std::set<uint32_t> in_round;
            EXPECT(!round.empty());
            for (const ShardPair& p : round) {
                EXPECT(p.first < S && p.second < S && p.first != p.second);
                EXPECT(in_round.insert(p.first).second);
                EXPECT(in_round.insert(p.second).second);
                EXPECT(seen.insert({std::min(p.first, p.second), std::max(p.first, p.second)}).second);
                ++row_side[p.first];
            }
        }
        EXPECT(seen.size() == (size_t)S * (S - 1) / 2);
        EXPECT(rounds.size() == (S < 2 ? 0u : S - 1 + (S & 1u)));   // the circle method's count
        // a shard is the row side of half of its S - 1 pairs, give or take one
        for (uint32_t s = 0; s < S; ++s) EXPECT(2 * row_side[s] + 2 >= S - 1 && 2 * row_side[s] <= S - 1 + 2);
    }
}

// the rectangles cover exactly the tiles that hold a qualifying element, each once
static void rects() {
    const uint64_t sizes[] = {0, 1, 127, 128, 129, 255, 256, 300, 640};
    for (uint64_t n_a : sizes)
        for (uint64_t n_b : sizes) {
            std::vector<uint64_t> fas = {0, 1, 127, 128, 129, n_a / 2, n_a ? n_a - 1 : 0, n_a};
            std::vector<uint64_t> fbs = {0, 1, 127, 128, 200, n_b / 2, n_b ? n_b - 1 : 0, n_b};
            for (uint64_t fn_a : fas)
                for (uint64_t fn_b : fbs) {
                    if (fn_a > n_a || fn_b > n_b) continue;
                    TileRect r[2];
                    const uint32_t n = between_rects(n_a, n_b, fn_a, fn_b, r);
                    const uint32_t nba = between_tiles_of(n_a), nbb = between_tiles_of(n_b);
                    std::vector<int> launched((size_t)nba * nbb, 0);
                    for (uint32_t i = 0; i < n; ++i) {
                        EXPECT(r[i].r0 < r[i].r1 && r[i].c0 < r[i].c1 && r[i].r1 <= nba && r[i].c1 <= nbb);
                        for (uint32_t bi = r[i].r0; bi < r[i].r1; ++bi)
                            for (uint32_t bj = r[i].c0; bj < r[i].c1; ++bj) ++launched[(size_t)bi * nbb + bj];
                    }
                    for (uint32_t bi = 0; bi < nba; ++bi)
                        for (uint32_t bj = 0; bj < nbb; ++bj) {
                            bool any = false;   // brute force: some element (ra, cb) of the tile with ra >= fn_a or cb >= fn_b
                            for (uint64_t ra = (uint64_t)bi * BETWEEN_TILE; ra < std::min<uint64_t>(n_a, (uint64_t)(bi + 1) * BETWEEN_TILE) && !any; ++ra)
                                for (uint64_t cb = (uint64_t)bj * BETWEEN_TILE; cb < std::min<uint64_t>(n_b, (uint64_t)(bj + 1) * BETWEEN_TILE); ++cb)
                                    if (ra >= fn_a || cb >= fn_b) { any = true; break; }
                            EXPECT(launched[(size_t)bi * nbb + bj] == (any ? 1 : 0));
                        }
                }
        }
    // 0, 0: one rectangle, everything
    TileRect r[2];
    EXPECT(between_rects(300, 500, 0, 0, r) == 1 && r[0].r0 == 0 && r[0].r1 == 3 && r[0].c0 == 0 && r[0].c1 == 4);
    EXPECT(between_rects(300, 500, 300, 500, r) == 0);
}

// a shard's local first_new = the number of its rows whose global id is below the bound
static void first_new() {
    const uint32_t blocks[] = {1, 3, 128, 256, 1000};
    const uint32_t shard_counts[] = {1, 2, 3, 4, 8};
    const uint64_t totals[] = {0, 1, 255, 256, 257, 1000, 2999, 4096};
    for (uint32_t block : blocks)
        for (uint32_t n : shard_counts)
            for (uint64_t total : totals) {
                std::vector<uint64_t> below(n, 0);   // rows of shard s with id < r, as r walks up
                for (uint64_t r = 0; r <= total; ++r) {
                    for (uint32_t s = 0; s < n; ++s) {
                        const uint64_t got = shard_first_new(block, n, s, r);
                        EXPECT(got == below[s]);
                        // ... and it is the local row of the first id >= r on that shard
                        if (got < cyclic_rows_of(block, n, s, total)) EXPECT(id_of_local(IdMap{0, block, n, s}, got) >= r);
                        if (got > 0) EXPECT(id_of_local(IdMap{0, block, n, s}, got - 1) < r || r == 0);
                    }
                    if (r < total) {
                        uint32_t s; uint64_t local;
                        cyclic_place(block, n, r, &s, &local);
                        EXPECT(local == below[s]);
                        ++below[s];
                    }
                }
            }
}

static void chunks() {
    EXPECT(between_chunk_rows(768, 0) == (256ull << 20) / (768 * 4) / 128 * 128);
    EXPECT(between_chunk_rows(768, 0) % BETWEEN_TILE == 0 && (uint64_t)between_chunk_rows(768, 0) * 768 * 4 <= BETWEEN_STAGE_BYTES);
    EXPECT(between_chunk_rows(768, 1) == 128 && between_chunk_rows(768, 128) == 128 && between_chunk_rows(768, 129) == 256);
    EXPECT(between_chunk_rows(1024, 0, 1000) == 128);   // a budget below one tile still stages one
    EXPECT(between_chunk_rows(128, 0) == (256ull << 20) / (128 * 4));
    const uint64_t sizes[] = {0, 1, 127, 128, 129, 1459, 4096, 100000};
    const uint32_t rows[] = {128, 256, 640, 87296};
    for (uint64_t n_b : sizes)
        for (uint32_t cr : rows) {
            const uint32_t n = between_n_chunks(n_b, cr);
            uint64_t at = 0;
            for (uint32_t i = 0; i < n; ++i) {
                uint64_t c0, c1;
                between_chunk(n_b, cr, i, &c0, &c1);
                EXPECT(c0 == at && c1 > c0 && c1 - c0 <= cr && c0 % BETWEEN_TILE == 0);
                if (i + 1 < n) EXPECT(c1 - c0 == cr);
                at = c1;
                // the bound of B as a bound of the chunk
                for (uint64_t fn : {(uint64_t)0, c0, c0 + 1, c1 - 1, c1, n_b}) {
                    const uint32_t cf = between_chunk_bound(fn, c0, c1);
                    for (uint64_t r = c0; r < c1; r += std::max<uint64_t>(1, (c1 - c0) / 7)) EXPECT((r >= fn) == (r - c0 >= cf));
                    EXPECT(cf <= c1 - c0);
                }
            }
            EXPECT(at == n_b);
        }
    EXPECT(between_n_chunks(1459, 640) == 3);   // two whole chunks and a ragged last one
    EXPECT(between_strip(1) == 256 && between_strip(1u << 12) == 64 && between_strip(1u << 20) == 1 && between_strip(0) == 256);
}

// the one strip walk: the rectangles it hands out, the halving after an overflow, stop(), the empty grounds
static void strips() {
    struct Call { uint32_t r0, r1, c0, c1; };
    const auto never = [] { return false; };
    // the rectangles tile [r0, r1) x [c0, c1) exactly once, whole column ranges, in ascending strips of between_strip(c1 - c0) rows
    const uint32_t grounds[][4] = {{0, 1, 0, 1}, {0, 3, 0, 3}, {5, 700, 2, 9}, {0, 1000, 0, 2048}, {3, 40, 7, 7 + (1u << 17)}, {0, 5, 0, 1u << 20}};
    for (const auto& g : grounds) {
        std::vector<Call> calls;
        tile_strips(g[0], g[1], g[2], g[3], [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool*) { calls.push_back(Call{a, b, c, d}); }, never);
        uint32_t at = g[0];
        for (size_t i = 0; i < calls.size(); ++i) {
            const Call& k = calls[i];
            EXPECT(k.r0 == at && k.r1 > k.r0 && k.c0 == g[2] && k.c1 == g[3]);
            EXPECT(k.r1 - k.r0 == between_strip(g[3] - g[2]) || (i + 1 == calls.size() && k.r1 - k.r0 < between_strip(g[3] - g[2])));
            at = k.r1;
        }
        EXPECT(at == g[1]);
    }
    // *overflowed is false on entry; a reported overflow halves the strips that follow, never below one tile row, and the
    // walk still covers every row once
    {
        std::vector<Call> calls;
        uint32_t n = 0;
        tile_strips(0, 1000, 0, 4096, [&](uint32_t a, uint32_t b, uint32_t, uint32_t, bool* over) {
            EXPECT(!*over);
            calls.push_back(Call{a, b, 0, 0});
            if (n++ < 9) *over = true;   // nine overflows from a strip of 64: 64, 32, 16, 8, 4, 2, 1, 1, 1, then 1 for good
        }, never);
        const uint32_t want[] = {64, 32, 16, 8, 4, 2, 1, 1, 1, 1, 1};
        EXPECT(calls.size() > 11);
        uint32_t at = 0;
        for (size_t i = 0; i < calls.size(); ++i) {
            EXPECT(calls[i].r0 == at && calls[i].r1 - calls[i].r0 == (i < 11 ? want[i] : 1u));
            at = calls[i].r1;
        }
        EXPECT(at == 1000);
    }
    {   // an overflow in the middle only: the strips before it keep their height, those after it have half
        std::vector<uint32_t> heights;
        tile_strips(0, 1024, 0, 1024, [&](uint32_t a, uint32_t b, uint32_t, uint32_t, bool* over) {
            heights.push_back(b - a);
            if (heights.size() == 2) *over = true;
        }, never);
        EXPECT(heights.size() == 6 && heights[0] == 256 && heights[1] == 256 && heights[2] == 128 && heights[5] == 128);
    }
    // stop() is asked before every strip and ends the walk between strips
    {
        uint32_t n = 0, asked = 0;
        tile_strips(0, 1000, 0, 4096, [&](uint32_t, uint32_t, uint32_t, uint32_t, bool*) { ++n; }, [&] { ++asked; return n == 3; });
        EXPECT(n == 3 && asked == 4);
        n = 0;
        tile_strips(0, 1000, 0, 4096, [&](uint32_t, uint32_t, uint32_t, uint32_t, bool*) { ++n; }, [] { return true; });
        EXPECT(n == 0);
    }
    // an empty ground calls nothing
    {
        uint32_t n = 0;
        const auto count = [&](uint32_t, uint32_t, uint32_t, uint32_t, bool*) { ++n; };
        tile_strips(7, 7, 0, 10, count, never);
        tile_strips(0, 10, 4, 4, count, never);
        tile_strips(9, 3, 0, 10, count, never);
        tile_strips(0, 10, 8, 2, count, never);
        EXPECT(n == 0);
    }
}

int main() {
    args();
    schedule();
    rects();
    first_new();
    chunks();
    strips();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
