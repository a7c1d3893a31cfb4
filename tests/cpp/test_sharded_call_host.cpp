// The part of image_search_amd/csrc/sharded_call.h without HIP in it, as a stand-alone program.
//   * the router against a brute-force placement through cyclic_place: per-shard ids in the list's order, positions that
//     scatter back to the identity, the empty list, the null list in both meanings, a list that leaves a shard empty (an empty
//     set, not a null pointer), and a bad id in the last position (the call's code and message, nothing dealt);
//   * the per-shard lists and their merge — through mi::merge_lists itself, which lives in that header — against a plain sort
//     by (distance key, id): equal distances across shards, NaN distances, MI_KNN_NO_ID padding, several queries; the counters'
//     column sums.
// Built with -fsanitize=address,undefined (tests/test_sharded_call_host.py); every array is heap memory of its exact size.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../image_search_amd/csrc/sharded_call.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

// the route of `ids` (never null here) against a placement of every entry by cyclic_place
static void expect_route(const ShardRoute& r, uint32_t block, uint32_t n, const std::vector<uint64_t>& ids) {
    EXPECT(r.listed);
    EXPECT(r.ids.size() == n && r.at.size() == n);
    std::vector<std::vector<uint64_t>> want(n), want_at(n);
    for (size_t i = 0; i < ids.size(); ++i) {
        uint32_t s = ~0u;
        uint64_t local = 0;
        cyclic_place(block, n, ids[i], &s, &local);
        want[s].push_back(ids[i]);
        want_at[s].push_back(i);
    }
    std::vector<uint64_t> back(ids.size(), ~0ull);
    size_t dealt = 0;
    for (uint32_t s = 0; s < n; ++s) {
        EXPECT(r.ids[s] == want[s]);        // the list's order inside every shard
        EXPECT(r.at[s] == want_at[s]);
        EXPECT(r.n_of(s) == want[s].size());
        EXPECT(r.of(s) != nullptr);         // a shard that holds none: an empty set, never "no list"
        if (!want[s].empty()) EXPECT(r.of(s) == r.ids[s].data());
        for (size_t j = 0; j < r.ids[s].size() && j < r.at[s].size(); ++j) {
            if (r.at[s][j] < back.size()) back[r.at[s][j]] = r.ids[s][j];
            ++dealt;
        }
    }
    EXPECT(dealt == ids.size());
    EXPECT(back == ids);                    // the positions scatter back to the identity
    size_t visited = 0;
    r.each([&](uint32_t s, const std::vector<uint64_t>& mine, const std::vector<uint64_t>& at) {
        EXPECT(!mine.empty() && mine == want[s] && at == want_at[s]);
        ++visited;
    });
    size_t holding = 0;
    for (uint32_t s = 0; s < n; ++s) holding += want[s].empty() ? 0 : 1;
    EXPECT(visited == holding);
}

static void router(uint32_t n, uint32_t block) {
    const uint64_t rows = (uint64_t)block * n * 2 + block / 2 + 7;   // two rounds of blocks and a ragged one
    // a shuffled list with duplicates
    std::vector<uint64_t> ids(3000);
    for (uint64_t& v : ids) v = rnd() % rows;
    for (size_t i = 0; i < 300; ++i) ids[rnd() % ids.size()] = ids[rnd() % ids.size()];
    ids.push_back(rows - 1);
    ids.push_back(0);
    expect_route(route_ids(block, n, rows, ids.data(), ids.size(), NULL_IS_NO_LIST), block, n, ids);
    expect_route(route_ids(block, n, rows, ids.data(), ids.size(), NULL_IS_FIRST_ROWS), block, n, ids);

    // an empty list is a list: every shard gets an empty set
    const uint64_t nothing = 0;
    expect_route(route_ids(block, n, rows, &nothing, 0, NULL_IS_NO_LIST), block, n, {});

    // a null list: "no list" ...
    const ShardRoute none = route_ids(block, n, rows, nullptr, 0, NULL_IS_NO_LIST);
    EXPECT(!none.listed && none.ids.size() == n);
    for (uint32_t s = 0; s < n; ++s) EXPECT(none.of(s) == nullptr && none.n_of(s) == 0);
    // ... or the first n rows
    std::vector<uint64_t> first(rows - 3);
    for (size_t i = 0; i < first.size(); ++i) first[i] = i;
    expect_route(route_ids(block, n, rows, nullptr, first.size(), NULL_IS_FIRST_ROWS), block, n, first);
    expect_route(route_ids(block, n, rows, nullptr, 0, NULL_IS_FIRST_ROWS), block, n, {});
    try {
        (void)route_ids(block, n, rows, nullptr, rows + 1, NULL_IS_FIRST_ROWS);
        EXPECT(!"more rows than the table holds must fail");
    } catch (const Error& e) {
        EXPECT(e.code == MI_ERR_INVALID);
    }

    // a list that leaves the last shard empty
    if (n > 1) {
        std::vector<uint64_t> some;
        for (uint64_t id : ids) {
            uint32_t s; uint64_t local;
            cyclic_place(block, n, id, &s, &local);
            if (s != n - 1) some.push_back(id);
        }
        const ShardRoute r = route_ids(block, n, rows, some.data(), some.size(), NULL_IS_NO_LIST);
        expect_route(r, block, n, some);
        EXPECT(r.n_of(n - 1) == 0 && r.of(n - 1) != nullptr);
    }

    // a bad id in the last position: the call's code and message, nothing dealt
    std::vector<uint64_t> bad(ids);
    bad.push_back(rows);
    for (NullList m : {NULL_IS_NO_LIST, NULL_IS_FIRST_ROWS}) {
        ShardRoute r;
        try {
            r = route_ids(block, n, rows, bad.data(), bad.size(), m);
            EXPECT(!"an id that is no row must fail");
        } catch (const Error& e) {
            char want[128];
            std::snprintf(want, sizeof want, "id %llu is not a row of this table (%llu rows)", (unsigned long long)rows, (unsigned long long)rows);
            EXPECT(e.code == MI_ERR_INVALID);
            EXPECT(std::string(e.what()) == want);
        }
        EXPECT(r.ids.empty() && r.at.empty() && !r.listed);
    }
}

static uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// 3 shards x nq queries x k entries -> [nq][k], against a plain sort by (distance key, id)
static void lists(uint32_t nq, uint32_t k) {
    const uint32_t n = 3;
    struct Ent { uint32_t key; uint64_t id; float d; };
    auto before = [](const Ent& a, const Ent& b) { return a.key < b.key || (a.key == b.key && a.id < b.id); };
    const float some_dist[] = {0.0f, -0.0f, 0.25f, 0.25f, 0.5f, 1.0f, 1.0f, 2.0f, -1.0f, NAN, INFINITY};   // few values: ties across shards
    ShardLists<int64_t> all(n, nq, k, 4, true);
    EXPECT(all.all_idx.size() == (size_t)n * nq * k && all.all_dist.size() == all.all_idx.size() && all.all_extra.size() == all.all_idx.size());
    EXPECT(all.all_counts.size() == (size_t)n * 4);
    std::vector<std::vector<Ent>> want(nq);
    for (uint32_t si = 0; si < n; ++si) {
        EXPECT(all.idx(si) == all.all_idx.data() + (size_t)si * nq * k);
        EXPECT(all.dist(si) == all.all_dist.data() + (size_t)si * nq * k);
        EXPECT(all.extra(si) == all.all_extra.data() + (size_t)si * nq * k);
        for (uint32_t u = 0; u < nq; ++u) {
            // a shard's list as a shard leaves it: its hits ascending by (key, id), padding behind; shard 1 finds fewer than k
            const uint32_t hits = si == 1 ? (uint32_t)(rnd() % (k + 1)) : k;
            std::vector<Ent> mine(hits);
            for (uint32_t j = 0; j < hits; ++j) {
                const float d = some_dist[rnd() % (sizeof some_dist / sizeof some_dist[0])];
                mine[j] = Ent{page_dist_key(d), (rnd() % 1000) * n + si, d};   // ids of shard si only (twice in one list does no harm)
            }
            std::sort(mine.begin(), mine.end(), before);
            for (uint32_t j = 0; j < k; ++j) {
                all.idx(si)[(size_t)u * k + j] = j < hits ? mine[j].id : MI_KNN_NO_ID;
                all.dist(si)[(size_t)u * k + j] = j < hits ? mine[j].d : INFINITY;
                all.extra(si)[(size_t)u * k + j] = (int64_t)si;
            }
            want[u].insert(want[u].end(), mine.begin(), mine.end());
        }
        for (uint32_t c = 0; c < 4; ++c) all.counts(si)[c] = 10 * si + c;
    }
    std::vector<uint64_t> idx((size_t)nq * k, 7);
    std::vector<float> dist((size_t)nq * k, 7.0f);
    merge_shard_lists(all, idx.data(), dist.data());
    for (uint32_t u = 0; u < nq; ++u) {
        std::stable_sort(want[u].begin(), want[u].end(), before);
        for (uint32_t j = 0; j < k; ++j) {
            const size_t o = (size_t)u * k + j;
            if (j < want[u].size()) {
                EXPECT(idx[o] == want[u][j].id);
                EXPECT(bits_of(dist[o]) == bits_of(want[u][j].d));   // (a key stands for one bit pattern here: NaN is NAN alone)
            } else {
                EXPECT(idx[o] == MI_KNN_NO_ID && dist[o] == INFINITY);
            }
        }
    }
    uint64_t sums[4] = {9, 9, 9, 9};
    all.sum_counts(sums);
    for (uint32_t c = 0; c < 4; ++c) EXPECT(sums[c] == (0 + 10 + 20) + 3 * c);

    // no lists, counters only (the stamp histogram's bins)
    ShardLists<> bins(n, 0, 0, 5);
    EXPECT(bins.all_idx.empty() && bins.all_dist.empty() && bins.all_extra.empty() && bins.all_counts.size() == 15);
    for (uint32_t si = 0; si < n; ++si)
        for (uint32_t c = 0; c < 5; ++c) bins.counts(si)[c] = si + c;
    uint64_t hist[5];
    bins.sum_counts(hist);
    for (uint32_t c = 0; c < 5; ++c) EXPECT(hist[c] == 3 + 3 * c);
}

int main() {
    const uint32_t layouts[][2] = {{1, 64}, {2, 64}, {3, 128}, {8, 64}, {5, 4096}};   // (shards, block)
    for (const auto& l : layouts) router(l[0], l[1]);
    for (uint32_t nq : {1u, 5u})
        for (uint32_t k : {1u, 7u, 64u}) lists(nq, k);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
