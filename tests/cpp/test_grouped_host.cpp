// The host-only pieces of mi_knn_search_grouped (image_search_amd/csrc/grouped_host.h) as a stand-alone program: the argument
// rules, the rule for group ids, the choice of the reduce form and its grid, the record's layout and the copy into caller
// arrays of exactly k elements (nullable ones left alone), the sharded merge by group id against a brute-force restatement,
// the sums over the shards' counts, and the directory -> group rule of the index.  Built with -fsanitize=address,undefined
// (tests/test_grouped_host.py); every array is heap memory of its exact size, so a read or write one element too far is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../image_search_amd/csrc/grouped_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static const uint64_t NO = MI_KNN_NO_ID;
static const uint32_t NG = MI_KNN_NO_GROUP;

static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    const float v[4] = {0, 0, 0, 0};
    const uint64_t ids[1] = {0};
    auto chk = [&](const void* tt, const float* q, uint32_t k, float md, const void* among, uint64_t n_among, const void* idx,
                   const void* dist) { return grouped_check_args(tt, q, k, md, among, n_among, idx, dist, &why); };
    EXPECT(chk(&t, v, 1, INFINITY, nullptr, 0, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 4096, 0.5f, ids, 1, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 64, -INFINITY, ids, 0, &o, &o) == MI_OK);            // an empty set; a bound below everything
    EXPECT(chk(nullptr, v, 1, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, nullptr, 1, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, INFINITY, nullptr, 0, nullptr, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, INFINITY, nullptr, 0, &o, nullptr) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, INFINITY, nullptr, 3, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, NAN, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 0, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 4097, INFINITY, nullptr, 0, &o, &o) == MI_ERR_UNSUPPORTED);
    EXPECT(chk(&t, v, 4097, NAN, nullptr, 0, &o, &o) == MI_ERR_INVALID);    // the bound is judged before k
    EXPECT(why && why[0] != '\0');

    EXPECT(grouped_id_ok(0) && grouped_id_ok(MI_KNN_GROUPS_MAX - 1) && grouped_id_ok(NG));
    EXPECT(!grouped_id_ok(MI_KNN_GROUPS_MAX) && !grouped_id_ok(0xFFFFFFFEu));
    std::vector<uint32_t> g = {0, 5, NG, MI_KNN_GROUPS_MAX - 1};
    EXPECT(grouped_first_bad(g.data(), g.size()) == g.size());
    g.push_back(MI_KNN_GROUPS_MAX);
    g.push_back(7);
    EXPECT(grouped_first_bad(g.data(), g.size()) == 4);
    EXPECT(grouped_first_bad(nullptr, 0) == 0);
}

static void forms_and_grid() {
    EXPECT(!grouped_use_lds(0, 4096));                 // no group: no reduce pass at all
    EXPECT(grouped_use_lds(1, 4096) && grouped_use_lds(4096, 4096) && !grouped_use_lds(4097, 4096));
    EXPECT(!grouped_use_lds(1, 0));                    // 0 forces the global form
    EXPECT(grouped_use_lds(300, 300) && !grouped_use_lds(301, 300));
    EXPECT(!grouped_use_lds(5000, 100000));            // the option cannot raise the LDS the kernel may ask for
    EXPECT((size_t)GROUP_LDS_MAX * GROUP_SLOT_BYTES == 48 * 1024);
    EXPECT(grouped_grid(1, 256, 0) == 1 && grouped_grid(256, 256, 0) == 1 && grouped_grid(257, 256, 0) == 2);
    EXPECT(grouped_grid(10'000'000, 256, 0) == 1024);
    EXPECT(grouped_grid(10'000'000, 256, 3) == 3 && grouped_grid(1000, 256, 1000) == 4 && grouped_grid(0, 256, 7) == 1);
    EXPECT(grouped_grid(0xFFFFFFFFull, 0, 0) == 4);
}

static void record() {
    for (uint32_t k : {1u, 3u, 64u, 65u, 4096u}) {
        const GroupedRecord r = grouped_record(k);
        EXPECT(r.idx == 0 && r.totals == 8u * k && r.members == r.totals + 32 && r.dist == r.members + 8u * k);
        EXPECT(r.group == r.dist + 4u * k && r.bytes == 24u * k + 32);
        EXPECT(r.totals % 8 == 0 && r.members % 8 == 0 && r.dist % 4 == 0 && r.group % 4 == 0);
        std::vector<unsigned char> rec(r.bytes);
        for (uint32_t j = 0; j < k; ++j) {
            const uint64_t id = 1000 + j, m = 3 + j;
            const float d = 0.5f + (float)j;
            const uint32_t g = j % 2 ? NG : j;
            std::memcpy(&rec[r.idx + 8u * j], &id, 8);
            std::memcpy(&rec[r.members + 8u * j], &m, 8);
            std::memcpy(&rec[r.dist + 4u * j], &d, 4);
            std::memcpy(&rec[r.group + 4u * j], &g, 4);
        }
        const uint64_t tot[4] = {11, 22, 33, 44};
        std::memcpy(&rec[r.totals], tot, 32);
        std::vector<uint64_t> idx(k), members(k), totals(4);
        std::vector<float> dist(k);
        std::vector<uint32_t> group(k);
        grouped_unpack(rec.data(), k, idx.data(), dist.data(), group.data(), members.data(), totals.data());
        EXPECT(idx[k - 1] == 1000 + k - 1 && members[k - 1] == 3 + k - 1 && dist[0] == 0.5f && group[0] == 0 && totals[3] == 44);
        if (k > 1) EXPECT(group[1] == NG);
        grouped_unpack(rec.data(), k, idx.data(), dist.data(), nullptr, nullptr, nullptr);   // the nullable outputs
        grouped_pad(k, idx.data(), dist.data(), group.data(), members.data(), totals.data());
        EXPECT(idx[0] == NO && idx[k - 1] == NO && std::isinf(dist[k - 1]) && group[k - 1] == NG && members[k - 1] == 0);
        EXPECT(totals[0] == 0 && totals[1] == 0 && totals[2] == 0 && totals[3] == 0);
        grouped_pad(k, idx.data(), dist.data(), nullptr, nullptr, nullptr);
    }
}

// the restatement of the merge: every entry of every list, the best (key, id) per group, singletons as they are
static void merge_against_brute_force() {
    uint64_t state = 12345;
    auto rnd = [&] { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
    for (int round = 0; round < 200; ++round) {
        const uint32_t n_lists = 1 + rnd() % 4, k = 1 + rnd() % 9;
        std::vector<uint64_t> idx((size_t)n_lists * k, NO);
        std::vector<float> dist((size_t)n_lists * k, INFINITY);
        std::vector<uint32_t> group((size_t)n_lists * k, NG);
        struct E { uint32_t key; uint64_t id; uint32_t g; };
        std::map<uint32_t, E> best;
        std::vector<E> singles;
        uint64_t next_id = 0;
        for (uint32_t l = 0; l < n_lists; ++l) {
            const uint32_t hits = rnd() % (k + 1);
            std::vector<uint32_t> used;
            for (uint32_t j = 0; j < hits; ++j) {
                const size_t e = (size_t)l * k + j;
                // few distinct distances (ties between lists), both zeros, a negative value
                const float choices[6] = {-0.25f, -0.0f, 0.0f, 0.125f, 0.5f, 2.0f};
                dist[e] = choices[rnd() % 6];
                idx[e] = next_id++ * 3 + rnd() % 3;
                uint32_t g = rnd() % 3 == 0 ? NG : rnd() % 5;
                for (uint32_t u : used)
                    if (u == g) g = NG;                   // a list holds a group once
                if (g != NG) used.push_back(g);
                group[e] = g;
                const E x{page_dist_key(dist[e]), idx[e], g};
                if (g == NG) singles.push_back(x);
                else {
                    auto it = best.find(g);
                    if (it == best.end() || x.key < it->second.key || (x.key == it->second.key && x.id < it->second.id)) best[g] = x;
                }
            }
        }
        std::vector<E> want = singles;
        for (auto& kv : best) want.push_back(kv.second);
        std::sort(want.begin(), want.end(), [](const E& a, const E& b) { return a.key != b.key ? a.key < b.key : a.id < b.id; });
        std::vector<uint64_t> o_idx(k);
        std::vector<float> o_dist(k);
        std::vector<uint32_t> o_group(k);
        grouped_merge(idx.data(), dist.data(), group.data(), n_lists, k, o_idx.data(), o_dist.data(), o_group.data());
        for (uint32_t j = 0; j < k; ++j) {
            if (j < want.size()) {
                EXPECT(o_idx[j] == want[j].id && o_group[j] == want[j].g && page_dist_key(o_dist[j]) == want[j].key);
            } else {
                EXPECT(o_idx[j] == NO && std::isinf(o_dist[j]) && o_dist[j] > 0 && o_group[j] == NG);
            }
        }
    }
    // the distance keeps its bits through the merge: -0 stays -0 and sorts before +0; the lower id wins a tie inside a group
    const uint64_t idx[4] = {9, 4, 7, NO};
    const float dist[4] = {0.0f, -0.0f, -0.0f, INFINITY};
    const uint32_t group[4] = {1, NG, 1, NG};
    uint64_t o_idx[2];
    float o_dist[2];
    uint32_t o_group[2];
    grouped_merge(idx, dist, group, 2, 2, o_idx, o_dist, o_group);
    EXPECT(o_idx[0] == 4 && o_idx[1] == 7 && bits_of(o_dist[0]) == 0x80000000u && bits_of(o_dist[1]) == 0x80000000u);
    EXPECT(o_group[0] == NG && o_group[1] == 1);
}

static void sums() {
    // shard 0: groups {0: 2, 2: 1} and 3 singletons (5 representatives); shard 1: groups {2: 4} and none (1); shard 2: nothing, a
    // shorter array
    const std::vector<std::vector<uint32_t>> cnt = {{2, 0, 1, 0}, {0, 0, 4, 0}, {0}};
    const uint64_t reps[3] = {5, 1, 0};
    std::vector<uint64_t> facets(4, 99);
    const uint64_t total = grouped_sum_counts(cnt, reps, 4, facets.data());
    EXPECT(total == 3 + 2);                            // the singletons, group 0, group 2 once
    EXPECT(facets[0] == 2 && facets[1] == 0 && facets[2] == 5 && facets[3] == 0);
    EXPECT(grouped_sum_counts(cnt, reps, 4, nullptr) == 5);
    EXPECT(grouped_sum_counts({}, nullptr, 0, nullptr) == 0);
}

static void directories() {
    EXPECT(grouped_dir_of("a/b/c.jpg") == "a/b/" && grouped_dir_of("a/b/d.jpg") == "a/b/" && grouped_dir_of("a/bb/c.jpg") == "a/bb/");
    EXPECT(grouped_dir_of("c.jpg").empty() && grouped_dir_of("/c.jpg") == "/" && grouped_dir_of("").empty());
    GroupDict d;
    EXPECT(d.of_path("/srv/media/x.jpg") == 0);       // directly in the media directory: one group
    EXPECT(d.of_path("/srv/media/a/b/c.jpg") == 1 && d.of_path("/srv/media/a/bb/c.jpg") == 2);
    EXPECT(d.of_path("/srv/media/a/b/d.jpg") == 1 && d.of_path("/srv/media/y.jpg") == 0 && d.of_path("/srv/media/a/e.jpg") == 3);
    EXPECT(d.names.size() == 4 && d.names[1] == "/srv/media/a/b/" && d.names[0] == "/srv/media/");
}

int main() {
    args();
    forms_and_grid();
    record();
    merge_against_brute_force();
    sums();
    directories();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
