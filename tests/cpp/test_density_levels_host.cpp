// The host-only pieces of mi_knn_density_levels / mi_knn_dbscan_levels / mi_dbscan_levels_tree
// (image_search_amd/csrc/density_levels_host.h) as a stand-alone program: the argument rules (every rejected case), the
// threshold struct and the level a distance falls into, and the tree builder against a brute-force restatement, with a
// disagreeing input and a cap below the edge count.  Built with -fsanitize=address,undefined
// (tests/test_density_levels_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../image_search_amd/csrc/density_levels_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    const float ok3[3] = {0.02f, 0.1f, 0.2f};
    const float eight[8] = {0.0f, 0.01f, 0.02f, 0.03f, 0.04f, 0.05f, 0.06f, INFINITY};
    const float nine[9] = {0.0f, 0.01f, 0.02f, 0.03f, 0.04f, 0.05f, 0.06f, 0.07f, 0.08f};
    EXPECT(density_levels_check_args(&t, ok3, 3, &o, &why) == MI_OK && why[0] == '\0');
    EXPECT(density_levels_check_args(&t, ok3, 1, &o, &why) == MI_OK);
    EXPECT(density_levels_check_args(&t, eight, 8, &o, &why) == MI_OK);             // 0 and +inf are numbers >= 0
    EXPECT(density_levels_check_args(nullptr, ok3, 3, &o, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(density_levels_check_args(&t, nullptr, 3, &o, &why) == MI_ERR_INVALID && std::strstr(why, "max_dists"));
    EXPECT(density_levels_check_args(&t, ok3, 3, nullptr, &why) == MI_ERR_INVALID && std::strstr(why, "counts"));
    EXPECT(density_levels_check_args(&t, ok3, 0, &o, &why) == MI_ERR_INVALID && std::strstr(why, "n_levels"));
    EXPECT(density_levels_check_args(&t, nine, 9, &o, &why) == MI_ERR_INVALID && std::strstr(why, "n_levels"));
    const float with_nan[3] = {0.02f, NAN, 0.2f}, first_nan[1] = {NAN}, negative[2] = {-0.1f, 0.1f};
    const float equal[3] = {0.02f, 0.1f, 0.1f}, falling[3] = {0.02f, 0.2f, 0.1f}, zeros[2] = {-0.0f, 0.0f};
    EXPECT(density_levels_check_args(&t, with_nan, 3, &o, &why) == MI_ERR_INVALID);
    EXPECT(density_levels_check_args(&t, first_nan, 1, &o, &why) == MI_ERR_INVALID && std::strstr(why, ">= 0"));
    EXPECT(density_levels_check_args(&t, negative, 2, &o, &why) == MI_ERR_INVALID && std::strstr(why, ">= 0"));
    EXPECT(density_levels_check_args(&t, equal, 3, &o, &why) == MI_ERR_INVALID && std::strstr(why, "ascending"));
    EXPECT(density_levels_check_args(&t, falling, 3, &o, &why) == MI_ERR_INVALID && std::strstr(why, "ascending"));
    EXPECT(density_levels_check_args(&t, zeros, 2, &o, &why) == MI_ERR_INVALID);    // -0 == +0: an equal pair
    EXPECT(density_levels_check_args(&t, equal, 2, &o, &why) == MI_OK);             // only the first n_levels are read

    EXPECT(dbscan_levels_check_args(&t, ok3, 3, 1, &o, &o, &why) == MI_OK && why[0] == '\0');
    EXPECT(dbscan_levels_check_args(&t, ok3, 3, 0xFFFFFFFFu, &o, &o, &why) == MI_OK);
    EXPECT(dbscan_levels_check_args(nullptr, ok3, 3, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, nullptr, 3, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, ok3, 0, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, nine, 9, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, with_nan, 3, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, negative, 2, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, equal, 3, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, falling, 3, 5, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, ok3, 3, 0, &o, &o, &why) == MI_ERR_INVALID && std::strstr(why, "min_pts"));
    EXPECT(dbscan_levels_check_args(&t, ok3, 3, 5, nullptr, &o, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_check_args(&t, ok3, 3, 5, &o, nullptr, &why) == MI_ERR_INVALID);
}

static void thresholds() {
    const float d3[3] = {0.02f, 0.1f, 0.2f};
    const DensityLevels lv = density_levels_make(d3, 3);
    EXPECT(lv.n == 3 && lv.d[0] == 0.02f && lv.d[1] == 0.1f && lv.d[2] == 0.2f);
    for (int j = 3; j < MI_KNN_LEVELS_MAX; ++j) EXPECT(lv.d[j] == 0.2f);
    EXPECT(density_level_of_host(lv, 0.0f) == 0 && density_level_of_host(lv, -0.0f) == 0 && density_level_of_host(lv, -1e-7f) == 0);
    EXPECT(density_level_of_host(lv, 0.02f) == 0);                                   // the bound is inclusive
    EXPECT(density_level_of_host(lv, std::nextafter(0.02f, 1.0f)) == 1);
    EXPECT(density_level_of_host(lv, 0.1f) == 1 && density_level_of_host(lv, 0.15f) == 2 && density_level_of_host(lv, 0.2f) == 2);
    EXPECT(density_level_of_host(lv, std::nextafter(0.2f, 1.0f)) == 3);              // in no level
    EXPECT(density_level_of_host(lv, NAN) == 3 && density_level_of_host(lv, INFINITY) == 3);
    // the level is the first one the single call's compare accepts, for every level and a sweep of distances
    for (int k = -5; k < 300; ++k) {
        const float dist = (float)k * 0.001f;
        uint32_t first = 3;
        for (uint32_t l = 3; l-- > 0;)
            if (dist <= d3[l]) first = l;
        EXPECT(density_level_of_host(lv, dist) == first);
    }
    const float one[1] = {0.5f};
    const DensityLevels l1 = density_levels_make(one, 1);
    EXPECT(l1.n == 1 && density_level_of_host(l1, 0.5f) == 0 && density_level_of_host(l1, 0.6f) == 1);
}

// the restatement: per level and cluster the set of parents its core rows name; one parent each, or the input is refused
static int brute_tree(const std::vector<uint64_t>& cluster, const std::vector<uint32_t>& counts, uint64_t rows, uint32_t L, uint32_t min_pts,
                      std::vector<LevelEdge>* out) {
    out->clear();
    for (uint32_t l = 0; l + 1 < L; ++l) {
        std::map<uint64_t, std::set<uint64_t>> parents;
        for (uint64_t r = 0; r < rows; ++r) {
            const uint64_t c = cluster[l * rows + r];
            if (c == MI_KNN_NO_ID || (uint64_t)counts[l * rows + r] + 1 < min_pts) continue;
            parents[c].insert(cluster[(l + 1) * rows + r]);
        }
        for (const auto& kv : parents) {
            if (kv.second.size() != 1 || *kv.second.begin() == MI_KNN_NO_ID) return MI_ERR_INVALID;
            out->push_back(LevelEdge{l, kv.first, *kv.second.begin()});
        }
    }
    return MI_OK;
}

static bool same(const std::vector<LevelEdge>& a, const std::vector<LevelEdge>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].level != b[i].level || a[i].child != b[i].child || a[i].parent != b[i].parent) return false;
    return true;
}

static void tree() {
    const uint64_t no = MI_KNN_NO_ID;
    const char* why = nullptr;
    std::vector<LevelEdge> got, want;
    // 3 levels x 8 rows, min_pts 3 (a core has counts >= 2).  Level 0: clusters 0 = {0, 1, 2} and 4 = {4, 5, 6}, 3 a border row
    // of 0, 7 noise.  Level 1: 3 has become a core, 7 a border row of 4.  Level 2: one cluster.
    const std::vector<uint64_t> cluster = {0, 0, 0, 0, 4, 4, 4, no,
                                           0, 0, 0, 0, 4, 4, 4, 4,
                                           0, 0, 0, 0, 0, 0, 0, 0};
    const std::vector<uint32_t> counts = {2, 2, 3, 1, 2, 2, 2, 0,
                                          2, 2, 3, 2, 2, 2, 3, 1,
                                          3, 3, 4, 3, 3, 3, 4, 2};
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, 3, 3, &got, &why) == MI_OK && why[0] == '\0');
    EXPECT(brute_tree(cluster, counts, 8, 3, 3, &want) == MI_OK && same(got, want));
    EXPECT(got.size() == 4 && got[0].level == 0 && got[0].child == 0 && got[0].parent == 0 && got[1].child == 4 && got[1].parent == 4);
    EXPECT(got[2].level == 1 && got[2].child == 0 && got[2].parent == 0 && got[3].level == 1 && got[3].child == 4 && got[3].parent == 0);
    // one level: no edges; no rows: no edges
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, 1, 3, &got, &why) == MI_OK && got.empty());
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 0, 3, 3, &got, &why) == MI_OK && got.empty());
    // a border row in a cluster that is not its lower cluster's parent changes nothing: 3 (a border row of 0) moves to 4 above
    std::vector<uint64_t> moved = cluster;
    std::vector<uint32_t> moved_counts = counts;
    moved[8 + 3] = 4; moved_counts[8 + 3] = 1;
    EXPECT(dbscan_levels_tree(moved.data(), moved_counts.data(), 8, 2, 3, &got, &why) == MI_OK && got.size() == 2);
    EXPECT(got[0].child == 0 && got[0].parent == 0 && got[1].child == 4 && got[1].parent == 4);
    // the cores of cluster 0 disagree about their parent: refused, and the output is left as it was
    std::vector<uint64_t> split = cluster;
    split[8 + 1] = 4;
    got.assign(1, LevelEdge{7, 7, 7});
    EXPECT(dbscan_levels_tree(split.data(), counts.data(), 8, 3, 3, &got, &why) == MI_ERR_INVALID && std::strstr(why, "two clusters"));
    EXPECT(got.size() == 1 && got[0].level == 7);
    EXPECT(brute_tree(split, counts, 8, 3, 3, &want) == MI_ERR_INVALID);
    // a core of level 0 in no cluster of level 1
    std::vector<uint64_t> lost = cluster;
    lost[8 + 5] = no;
    EXPECT(dbscan_levels_tree(lost.data(), counts.data(), 8, 3, 3, &got, &why) == MI_ERR_INVALID && std::strstr(why, "no cluster"));
    EXPECT(brute_tree(lost, counts, 8, 3, 3, &want) == MI_ERR_INVALID);
    // the argument rules of the builder itself
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, 0, 3, &got, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, MI_KNN_LEVELS_MAX + 1, 3, &got, &why) == MI_ERR_INVALID);
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, 3, 0, &got, &why) == MI_ERR_INVALID && std::strstr(why, "min_pts"));
    // min_pts decides who is a core: at 4 only rows 2 (and 6 above) are, at 1 every clustered row is
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, 3, 4, &got, &why) == MI_OK);
    EXPECT(brute_tree(cluster, counts, 8, 3, 4, &want) == MI_OK && same(got, want) && got.size() == 3);
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 8, 3, 1, &got, &why) == MI_OK);
    EXPECT(brute_tree(cluster, counts, 8, 3, 1, &want) == MI_OK && same(got, want));

    // random nested inputs against the restatement: level l + 1 merges the clusters of level l in random groups, so the cores
    // always agree; ids above 32 bits; then one core row is moved to break the agreement
    uint32_t seed = 2024u;
    auto rnd = [&](uint32_t m) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % m; };
    for (int round = 0; round < 200; ++round) {
        const uint64_t rows = 1 + rnd(40);
        const uint32_t L = 1 + rnd(MI_KNN_LEVELS_MAX), min_pts = 1 + rnd(4);
        const uint64_t base = round % 2 ? (1ull << 40) : 0;
        std::vector<uint64_t> cl(L * rows);
        std::vector<uint32_t> cn(L * rows);
        std::vector<uint32_t> group(rows);
        for (uint64_t r = 0; r < rows; ++r) group[r] = rnd(6);
        for (uint32_t l = 0; l < L; ++l) {
            if (l > 0) {
                uint32_t merge[6];
                for (uint32_t& m : merge) m = rnd(6);
                for (uint64_t r = 0; r < rows; ++r) group[r] = merge[group[r]];
            }
            for (uint64_t r = 0; r < rows; ++r) {
                cn[l * rows + r] = (l > 0 ? cn[(l - 1) * rows + r] : 0u) + rnd(3);   // degrees only grow with the level
                const bool clustered = (l > 0 && cl[(l - 1) * rows + r] != no) || rnd(4) != 0;
                cl[l * rows + r] = clustered ? base + group[r] : no;
            }
        }
        const int w = brute_tree(cl, cn, rows, L, min_pts, &want);
        EXPECT(w == MI_OK);
        EXPECT(dbscan_levels_tree(cl.data(), cn.data(), rows, L, min_pts, &got, &why) == w && same(got, want));
        for (size_t i = 1; i < got.size(); ++i)
            EXPECT(got[i - 1].level < got[i].level || (got[i - 1].level == got[i].level && got[i - 1].child < got[i].child));
        if (L >= 2 && rows >= 2) {
            const uint64_t r = rnd((uint32_t)rows);
            cl[rows + r] = base + 99;                                                 // a cluster nobody else is in
            const int w2 = brute_tree(cl, cn, rows, L, min_pts, &want);
            EXPECT(dbscan_levels_tree(cl.data(), cn.data(), rows, L, min_pts, &got, &why) == w2);
            if (w2 == MI_OK) EXPECT(same(got, want));
        }
    }
}

// mi_dbscan_levels_tree's cap convention as density_levels.hip applies it: the full count, the first cap edges
static void cap() {
    const uint64_t no = MI_KNN_NO_ID;
    const std::vector<uint64_t> cluster = {0, 0, 2, 2, 4, no,
                                           0, 0, 0, 0, 4, 4};
    const std::vector<uint32_t> counts = {1, 1, 1, 1, 0, 0,
                                          3, 3, 3, 3, 1, 1};
    const char* why = nullptr;
    std::vector<LevelEdge> edges;
    EXPECT(dbscan_levels_tree(cluster.data(), counts.data(), 6, 2, 1, &edges, &why) == MI_OK && edges.size() == 3);
    uint32_t level[2] = {9, 9};
    uint64_t child[2] = {9, 9}, parent[2] = {9, 9};
    const uint64_t capacity = 2;
    const size_t n = (size_t)std::min<uint64_t>(capacity, edges.size());
    for (size_t i = 0; i < n; ++i) { level[i] = edges[i].level; child[i] = edges[i].child; parent[i] = edges[i].parent; }
    EXPECT(n == 2 && edges.size() == 3 && child[0] == 0 && parent[0] == 0 && child[1] == 2 && parent[1] == 0 && level[1] == 0);
    EXPECT(edges[2].child == 4 && edges[2].parent == 4);
}

int main() {
    args();
    thresholds();
    tree();
    cap();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
