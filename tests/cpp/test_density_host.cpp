// The host-only pieces of mi_knn_density / mi_knn_dbscan / mi_index_themes (image_search_amd/csrc/density_host.h) as a
// stand-alone program: the argument rules, the tiles pass 2 visits and skips against a brute-force walk over every rectangle,
// the dense renumbering of the cluster ids and the cluster lists.  Built with -fsanitize=address,undefined
// (tests/test_density_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_search_amd/csrc/density_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    EXPECT(density_check_args(&t, 0.0f, &o, &why) == MI_OK && why[0] == '\0');
    EXPECT(density_check_args(&t, INFINITY, &o, &why) == MI_OK);
    EXPECT(density_check_args(nullptr, 0.1f, &o, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(density_check_args(&t, -0.1f, &o, &why) == MI_ERR_INVALID && std::strstr(why, "max_dist"));
    EXPECT(density_check_args(&t, NAN, &o, &why) == MI_ERR_INVALID);
    EXPECT(density_check_args(&t, 0.1f, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(density_check_args(&t, -0.0f, &o, &why) == MI_OK);   // -0 >= 0

    EXPECT(dbscan_check_args(&t, 0.1f, 1, &o, &o, &why) == MI_OK);
    EXPECT(dbscan_check_args(&t, 0.1f, 0xFFFFFFFFu, &o, &o, &why) == MI_OK);
    EXPECT(dbscan_check_args(nullptr, 0.1f, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 0, &o, &o, &why) == MI_ERR_INVALID && std::strstr(why, "min_pts"));
    EXPECT(dbscan_check_args(&t, NAN, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, -1.0f, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 5, nullptr, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_check_args(&t, 0.1f, 5, &o, nullptr, &why) == MI_ERR_INVALID);
}

static void tiles() {
    EXPECT(!density_tile_visited(0, 3) && !density_tile_visited(1, 1) && density_tile_visited(1, 3) && density_tile_visited(3, 1));
    EXPECT(density_tile_visited(3, 3) && !density_tile_visited(2, 3) && !density_tile_visited(1, 0));
    uint32_t seed = 12345u;
    for (uint32_t n = 1; n <= 13; ++n) {
        for (int round = 0; round < 8; ++round) {
            DensityBlocks b;
            b.act.resize(n);
            for (uint32_t j = 0; j < n; ++j) {
                seed = seed * 1664525u + 1013904223u;
                const uint8_t v = (uint8_t)((seed >> 24) & 3u);   // (2 alone happens: min_pts 1 makes a lone row a core)
                b.act[j] = v;
            }
            b.index();
            uint64_t tri_v = 0, tri_s = 0;
            for (uint32_t r0 = 0; r0 < n; ++r0)
                for (uint32_t r1 = r0 + 1; r1 <= n; ++r1)
                    for (uint32_t c0 = 0; c0 < n; ++c0)
                        for (uint32_t c1 = c0 + 1; c1 <= n; ++c1) {
                            uint64_t v = 0, s = 0, bv = 0, bs = 0;
                            b.count(r0, r1, c0, c1, &v, &s);
                            for (uint32_t bi = r0; bi < r1; ++bi)
                                for (uint32_t bj = c0 > bi ? c0 : bi; bj < c1; ++bj)
                                    (density_tile_visited(b.act[bi], b.act[bj]) ? bv : bs) += 1;
                            EXPECT(v == bv && s == bs);
                            if (r0 == 0 && r1 == n && c0 == 0 && c1 == n) { tri_v = v; tri_s = s; }
                        }
            EXPECT(tri_v + tri_s == (uint64_t)n * (n + 1) / 2);
        }
    }
}

static void labels() {
    const uint64_t no = MI_KNN_NO_ID;
    const uint64_t c[7] = {9, no, 3, 9, 1ull << 40, 3, no};
    int64_t lab[7];
    EXPECT(density_dense_labels(c, 7, lab) == 3);
    const int64_t want[7] = {1, -1, 0, 1, 2, 0, -1};
    EXPECT(std::memcmp(lab, want, sizeof want) == 0);
    EXPECT(density_dense_labels(c, 0, lab) == 0);
    const uint64_t none[2] = {no, no};
    EXPECT(density_dense_labels(none, 2, lab) == 0 && lab[0] == -1 && lab[1] == -1);
}

static void lists() {
    const uint64_t no = MI_KNN_NO_ID;
    // cluster 5 = {2, 5, 6} (2: a border row below the cluster's id), cluster 3 = {3, 4, 9}, rows 0, 1, 7, 8 in none
    const uint64_t cluster[10] = {no, no, 5, 3, 3, 5, 5, no, no, 3};
    uint64_t ids[10];
    for (int i = 0; i < 10; ++i) ids[i] = (uint64_t)i;
    std::vector<uint64_t> gids, starts;
    density_lists(ids, cluster, 10, &gids, &starts);
    EXPECT((gids == std::vector<uint64_t>{2, 5, 6, 3, 4, 9}));     // ordered by the smallest member, not by the cluster id
    EXPECT((starts == std::vector<uint64_t>{0, 3, 6}));
    // ids above 32 bits
    for (int i = 0; i < 10; ++i) ids[i] = (1ull << 40) + (uint64_t)i;
    uint64_t cl2[10];
    for (int i = 0; i < 10; ++i) cl2[i] = cluster[i] == no ? no : (1ull << 40) + cluster[i];
    density_lists(ids, cl2, 10, &gids, &starts);
    EXPECT(gids.size() == 6 && gids[0] == (1ull << 40) + 2 && gids[3] == (1ull << 40) + 3 && starts.size() == 3);
    density_lists(ids, cl2, 0, &gids, &starts);
    EXPECT(gids.empty() && (starts == std::vector<uint64_t>{0}));
    const uint64_t none[3] = {no, no, no};
    density_lists(ids, none, 3, &gids, &starts);
    EXPECT(gids.empty() && (starts == std::vector<uint64_t>{0}));
    const uint64_t one[1] = {7};
    const uint64_t id7[1] = {7};
    density_lists(id7, one, 1, &gids, &starts);
    EXPECT((gids == std::vector<uint64_t>{7}) && (starts == std::vector<uint64_t>{0, 1}));
}

int main() {
    args();
    tiles();
    labels();
    lists();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
