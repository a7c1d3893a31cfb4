// The host-only pieces of mi_knn_sharded_density / mi_knn_sharded_dbscan (image_search_amd/csrc/density_sharded_host.h) as a
// stand-alone program: the argument rules, the tiles a cross rectangle of pass 2 visits and skips against a brute-force walk
// over every rectangle, the scatter of the shards' local arrays to global rows for several layouts, and the forest merge
// against components found by a brute-force flood fill.  Built with -fsanitize=address,undefined
// (tests/test_density_sharded_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_search_amd/csrc/density_sharded_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint32_t seed = 2024u;
static uint32_t rnd() {
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
}

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    EXPECT(density_check_args(&t, 0.0f, &o, &why) == MI_OK && why[0] == '\0');
    EXPECT(density_check_args(nullptr, 0.1f, &o, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(density_check_args(&t, -0.1f, &o, &why) == MI_ERR_INVALID && std::strstr(why, "max_dist"));
    EXPECT(density_check_args(&t, NAN, &o, &why) == MI_ERR_INVALID);
    EXPECT(density_check_args(&t, 0.1f, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 1, &o, &o, &why) == MI_OK);
    EXPECT(dbscan_check_args(nullptr, 0.1f, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 0, &o, &o, &why) == MI_ERR_INVALID && std::strstr(why, "min_pts"));
    EXPECT(dbscan_check_args(&t, NAN, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, -1.0f, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 5, nullptr, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 5, &o, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(sharded_density_rows_ok(0) && sharded_density_rows_ok(0xFFFFFFFFull) && !sharded_density_rows_ok(1ull << 32));
}

static void cross_tiles() {
    for (uint32_t na = 1; na <= 7; ++na)
        for (uint32_t nb = 1; nb <= 7; ++nb)
            for (int round = 0; round < 4; ++round) {
                std::vector<uint8_t> row(na), col(nb);
                for (uint8_t& v : row) v = (uint8_t)(rnd() & 3u);
                for (uint8_t& v : col) v = (uint8_t)(rnd() & 3u);
                CrossBlocks b;
                b.index(col.data(), nb);
                for (uint32_t r0 = 0; r0 < na; ++r0)
                    for (uint32_t r1 = r0 + 1; r1 <= na; ++r1)
                        for (uint32_t c0 = 0; c0 < nb; ++c0)
                            for (uint32_t c1 = c0 + 1; c1 <= nb; ++c1) {
                                uint64_t v = 0, s = 0, bv = 0, bs = 0;
                                b.count(row.data(), r0, r1, c0, c1, &v, &s);
                                for (uint32_t bi = r0; bi < r1; ++bi)
                                    for (uint32_t bj = c0; bj < c1; ++bj) (density_tile_visited(row[bi], col[bj]) ? bv : bs) += 1;
                                EXPECT(v == bv && s == bs && v + s == (uint64_t)(r1 - r0) * (c1 - c0));
                            }
            }
    // a chunk inside a longer array of blocks: the prefix counts start at the chunk
    const uint8_t all[6] = {3, 0, 1, 3, 0, 1}, row[2] = {1, 3};
    CrossBlocks b;
    b.index(all + 2, 3);   // blocks 2, 3, 4: {1, 3, 0}
    uint64_t v = 0, s = 0;
    b.count(row, 0, 2, 0, 3, &v, &s);
    EXPECT(v == 3 && s == 3);   // row 0 (no core): only the column with a core; row 1 (core): both columns with a neighbour
    b.index(all, 0);
    b.count(row, 0, 2, 0, 0, &v, &s);
    EXPECT(v == 0 && s == 0);
}

static void scatter() {
    const uint32_t layouts[4][2] = {{3, 64}, {2, 128}, {4, 64}, {1, 64}};
    for (const auto& lay : layouts) {
        const uint32_t S = lay[0], block = lay[1];
        for (uint64_t total : {0ull, 1ull, 63ull, 64ull, 100ull, 1500ull}) {
            std::vector<uint64_t> out(total, ~0ull);
            uint64_t placed = 0;
            for (uint32_t s = 0; s < S; ++s) {
                const IdMap map{0, block, S, s};
                const uint64_t n = cyclic_rows_of(block, S, s, total);
                std::vector<uint64_t> local(n);
                for (uint64_t r = 0; r < n; ++r) local[r] = ((uint64_t)s << 32) | r;
                scatter_to_global(map, local.data(), n, out.data());   // (an id beyond `total` would write out of bounds: the sanitizer watches)
                placed += n;
            }
            EXPECT(placed == total);
            for (uint64_t g = 0; g < total; ++g) {
                uint32_t s;
                uint64_t local;
                cyclic_place(block, S, g, &s, &local);
                EXPECT(out[g] == (((uint64_t)s << 32) | local));
            }
        }
    }
}

// components of the union of the forests' links, by flood fill over an adjacency matrix
static std::vector<uint32_t> brute_roots(const std::vector<std::vector<uint32_t>>& forests, uint32_t G) {
    std::vector<uint8_t> adj((size_t)G * G, 0);
    for (const auto& f : forests)
        for (uint32_t g = 0; g < G; ++g) adj[(size_t)g * G + f[g]] = adj[(size_t)f[g] * G + g] = 1;
    std::vector<uint32_t> root(G, 0xFFFFFFFFu);
    for (uint32_t g = 0; g < G; ++g) {
        if (root[g] != 0xFFFFFFFFu) continue;
        std::vector<uint32_t> todo{g};   // g is the smallest row not yet reached: the component's smallest
        root[g] = g;
        while (!todo.empty()) {
            const uint32_t x = todo.back();
            todo.pop_back();
            for (uint32_t y = 0; y < G; ++y)
                if (adj[(size_t)x * G + y] && root[y] == 0xFFFFFFFFu) { root[y] = g; todo.push_back(y); }
        }
    }
    return root;
}

static void forests() {
    for (uint32_t G : {1u, 2u, 7u, 40u, 97u})
        for (uint32_t S = 1; S <= 4; ++S)
            for (int round = 0; round < 6; ++round) {
                // S forests with parent[x] <= x: each built by random unions under the smallest-root rule
                std::vector<std::vector<uint32_t>> fs(S, std::vector<uint32_t>(G));
                for (auto& f : fs) {
                    for (uint32_t g = 0; g < G; ++g) f[g] = g;
                    const uint32_t links = rnd() % (G + 1);
                    for (uint32_t i = 0; i < links; ++i) {
                        const uint32_t a = forest_find(f, rnd() % G), b = forest_find(f, rnd() % G);
                        if (a != b) f[a > b ? a : b] = a < b ? a : b;
                    }
                }
                const std::vector<uint32_t> want = brute_roots(fs, G);
                // merged in two orders: the same roots
                for (int order = 0; order < 2; ++order) {
                    std::vector<uint32_t> into = order == 0 ? fs[0] : fs[S - 1];
                    uint64_t merged = 0;
                    for (uint32_t k = 1; k < S; ++k) merged += forest_merge(into, order == 0 ? fs[k] : fs[S - 1 - k]);
                    uint32_t roots_before = 0, roots_after = 0;
                    for (uint32_t g = 0; g < G; ++g) {
                        EXPECT(into[g] <= g);
                        EXPECT(forest_find(into, g) == want[g]);
                        roots_before += (order == 0 ? fs[0] : fs[S - 1])[g] == g;
                        roots_after += want[g] == g;
                    }
                    EXPECT(merged == roots_before - roots_after);
                }
            }
}

int main() {
    args();
    cross_tiles();
    scatter();
    forests();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
