// A stand-alone program over image_search_amd/csrc/summary_sharded_host.h: the dealing of the caller's labels to the shards
// against cyclic_place, the per-group slots of every shard turned to global ids and merged (in two shard orders) against slots
// computed over the whole row set — equal keys on different shards, groups whose distances are all NaN, empty groups and
// shards that hold none of a group among them — and the bytes that cross between shards.  Built with the address and
// undefined-behaviour sanitizers by tests/test_summary_sharded_host.py; it needs neither the library nor a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../image_search_amd/csrc/density_sharded_host.h"   // scatter_to_global
#include "../../image_search_amd/csrc/summary_sharded_host.h"

using namespace mi;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static const uint32_t LAYOUTS[][2] = {{1, 64}, {2, 64}, {3, 128}, {8, 64}, {5, 4096}};   // (shards, block)

static uint64_t rows_of(uint32_t n, uint32_t block) { return (uint64_t)block * n * 2 + block / 2 + 7; }   // two rounds and a ragged one

// ---- the dealing ------------------------------------------------------------------------------------------------------------
static void test_deal(uint32_t n, uint32_t block) {
    const uint64_t G = rows_of(n, block);
    std::vector<uint32_t> labels(G);
    for (uint64_t r = 0; r < G; ++r) labels[r] = (uint32_t)(r * 2654435761u + 17u);   // every row another value
    std::vector<uint32_t> back(G, 0);
    uint64_t seen = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const IdMap map{0, block, n, s};
        const uint64_t mine = cyclic_rows_of(block, n, s, G);
        std::vector<uint32_t> local(mine + 1, 0xABABABABu);   // (+ 1: a guard behind the last row)
        summary_deal_labels(map, labels.data(), mine, local.data());
        CHECK(local[mine] == 0xABABABABu);
        for (uint64_t r = 0; r < G; ++r) {   // every global row the placement gives to s found its local row
            uint32_t at; uint64_t l;
            cyclic_place(block, n, r, &at, &l);
            if (at != s) continue;
            CHECK(l < mine && local[l] == labels[r]);
            ++seen;
        }
        scatter_to_global(map, local.data(), mine, back.data());   // ... and the scatter is its inverse
    }
    CHECK(seen == G);
    CHECK(back == labels);
}

// ---- the slots ----------------------------------------------------------------------------------------------------------------
struct Row { uint32_t label; float dist; };

// what summary_dist_kernel leaves for rows [0, n) named by `name(r)`: slots [4][C]
template <class Name>
static std::vector<uint64_t> slots_of(const std::vector<Row>& rows, uint32_t C, Name&& name) {
    std::vector<uint64_t> s((size_t)SUMMARY_PLANES * C, 0);
    for (uint32_t c = 0; c < C; ++c) s[c] = SUMMARY_MIN_INIT;
    for (size_t r = 0; r < rows.size(); ++r) {
        const uint32_t c = rows[r].label;
        if (c >= C) continue;
        const float d = rows[r].dist;
        const uint32_t key = summary_key_of(d), id = name(r);
        const uint64_t lo = summary_min_word(key, id);
        if (lo < s[c]) s[c] = lo;
        if (d == d) {
            const uint64_t hi = summary_max_word(key, id);
            if (hi > s[(size_t)C + c]) s[(size_t)C + c] = hi;
            s[(size_t)2 * C + c] += 1;
            s[(size_t)3 * C + c] += summary_weight(d);
        }
    }
    return s;
}

static void test_slots(uint32_t n, uint32_t block, uint32_t seed) {
    const uint64_t G = rows_of(n, block);
    const uint32_t C = 7;
    // group 0: a few distance values, so equal keys fall on different shards; 1: all NaN; 2: empty; 3: rows of the first block
    // only (one shard); 4: one value everywhere (every member ties); 5: NaN and numbers mixed; 6: a single row, on the last shard
    // that holds rows
    const float some[] = {0.0f, -0.0f, 0.25f, 0.25f, 0.5f, 1.0f, 2.0f, -1e-7f, INFINITY};
    std::mt19937 rnd(seed);
    std::vector<Row> all(G);
    for (uint64_t r = 0; r < G; ++r) {
        const uint32_t pick = rnd() % 8;
        Row x{0xFFFFFFFFu, 0.0f};   // (pick 2 and 7: belongs to nothing)
        if (pick == 0) x = Row{0, some[rnd() % 9]};
        else if (pick == 1) x = Row{1, NAN};
        else if (pick == 3 && r < block) x = Row{3, some[rnd() % 9]};
        else if (pick == 4) x = Row{4, 0.375f};
        else if (pick == 5) x = Row{5, (rnd() & 1) ? NAN : some[rnd() % 9]};
        else if (pick == 6) x = Row{9, 0.5f};   // a label >= C
        all[r] = x;
    }
    all[G - 1] = Row{6, 0.75f};
    const std::vector<uint64_t> want = slots_of(all, C, [](size_t r) { return (uint32_t)r; });

    // every shard's own slots over LOCAL rows, then to global ids
    std::vector<std::vector<uint64_t>> per(n);
    std::vector<uint32_t> count(C, 0);
    for (const Row& x : all)
        if (x.label < C) ++count[x.label];
    bool none_somewhere = false;
    for (uint32_t s = 0; s < n; ++s) {
        const IdMap map{0, block, n, s};
        const uint64_t mine = cyclic_rows_of(block, n, s, G);
        std::vector<Row> local(mine);
        for (uint64_t l = 0; l < mine; ++l) local[l] = all[id_of_local(map, l)];
        per[s] = slots_of(local, C, [](size_t r) { return (uint32_t)r; });
        if (per[s][3] == SUMMARY_MIN_INIT) none_somewhere = true;
        const std::vector<uint64_t> before = per[s];
        summary_globalize_slots(per[s].data(), C, map);
        // the same as naming the rows by their global ids in the first place
        CHECK(per[s] == slots_of(local, C, [&](size_t r) { return (uint32_t)id_of_local(map, r); }));
        for (uint32_t c = 0; c < C; ++c) {   // start values stay, the keys and the sums are untouched
            if (before[c] == SUMMARY_MIN_INIT) CHECK(per[s][c] == SUMMARY_MIN_INIT);
            if (before[C + c] == SUMMARY_MAX_INIT) CHECK(per[s][C + c] == SUMMARY_MAX_INIT);
            CHECK((per[s][c] >> 32) == (before[c] >> 32) && (per[s][C + c] >> 32) == (before[C + c] >> 32));
            CHECK(per[s][2 * C + c] == before[2 * C + c] && per[s][3 * C + c] == before[3 * C + c]);
        }
    }
    if (n > 1) CHECK(none_somewhere);   // group 3 lives on shard 0 alone

    for (int order = 0; order < 2; ++order) {
        std::vector<uint64_t> got = per[0];
        for (uint32_t i = 1; i < n; ++i) summary_merge_slots(got.data(), per[order == 0 ? i : n - i].data(), C);
        CHECK(got == want);
        // ... and decoded with the identity map: a word's row is the id
        std::vector<uint64_t> cover(C), odd(C), measured(C), spread(C);
        std::vector<float> cover_dist(C), odd_dist(C);
        summary_decode(got.data(), count.data(), C, IdMap{0, block, 1, 0}, cover.data(), cover_dist.data(), odd.data(), odd_dist.data(),
                       measured.data(), spread.data());
        for (uint32_t c = 0; c < C; ++c) {
            uint64_t best = MI_KNN_NO_ID, worst = MI_KNN_NO_ID;   // the rule itself: (key, id) ascending; (key desc, id asc)
            for (uint64_t r = 0; r < G; ++r) {
                if (all[r].label != c) continue;
                const uint32_t k = summary_key_of(all[r].dist);
                if (best == MI_KNN_NO_ID || k < summary_key_of(all[best].dist)) best = r;
                if (all[r].dist == all[r].dist && (worst == MI_KNN_NO_ID || k > summary_key_of(all[worst].dist))) worst = r;
            }
            CHECK(cover[c] == best && odd[c] == worst);
        }
        CHECK(cover[2] == MI_KNN_NO_ID && count[2] == 0);
        CHECK(count[1] > 0 && cover[1] != MI_KNN_NO_ID && cover_dist[1] != cover_dist[1] && odd[1] == MI_KNN_NO_ID && measured[1] == 0);
        CHECK(cover[6] == G - 1 && odd[6] == G - 1 && measured[6] == 1);
        // group 4: every member ties, the lowest global id wins on both ends whichever shard holds it
        uint64_t first4 = 0;
        while (all[first4].label != 4) ++first4;
        CHECK(cover[4] == first4 && odd[4] == first4 && measured[4] == count[4]);
    }
}

// the tie of the contract by hand: 3 shards of 64-row blocks, one distance at ids 60, 64, 130 and 200.  Row 64 is local row 0
// of shard 1: a merge that compared local rows would answer 64.
static void test_tie_by_hand() {
    const uint32_t n = 3, block = 64, C = 1;
    const uint64_t ids[] = {60, 64, 130, 200};
    std::vector<std::vector<uint64_t>> per(n, std::vector<uint64_t>{SUMMARY_MIN_INIT, SUMMARY_MAX_INIT, 0, 0});
    const uint32_t key = summary_key_of(0.5f);
    for (uint64_t id : ids) {
        uint32_t s; uint64_t l;
        cyclic_place(block, n, id, &s, &l);
        std::vector<uint64_t> one{summary_min_word(key, (uint32_t)l), summary_max_word(key, (uint32_t)l), 1, summary_weight(0.5f)};
        summary_merge_slots(per[s].data(), one.data(), C);   // (inside a shard the same rule holds, on local rows)
    }
    CHECK((uint32_t)per[1][0] == 0);   // id 64 IS local row 0 of shard 1
    for (uint32_t s = 0; s < n; ++s) summary_globalize_slots(per[s].data(), C, IdMap{0, block, n, s});
    std::vector<uint64_t> got = per[2];
    summary_merge_slots(got.data(), per[1].data(), C);
    summary_merge_slots(got.data(), per[0].data(), C);
    CHECK((uint32_t)got[0] == 60 && (uint32_t)~(uint32_t)got[1] == 60 && got[2] == 4 && got[3] == 4ull << 29);
}

static void test_bytes() {
    CHECK(summary_sharded_exchange_bytes(0, 5, 768) == 0);
    CHECK(summary_sharded_exchange_bytes(1, 5, 768) == 0);
    CHECK(summary_sharded_exchange_bytes(2, 1, 128) == (8 * 128 + 4 + 32) + 4 * 128);
    CHECK(summary_sharded_exchange_bytes(4, 20, 768) == 3ull * 20 * (8 * 768 + 36) + 3ull * 4 * 20 * 768);
    // no 32-bit product on the way: 64 shards, 65536 groups, dim 1024
    CHECK(summary_sharded_exchange_bytes(64, 65536, 1024) == 63ull * 65536 * (8ull * 1024 + 36) + 63ull * 4 * 65536 * 1024);
}

int main() {
    for (const auto& l : LAYOUTS) {
        test_deal(l[0], l[1]);
        test_slots(l[0], l[1], 7);
        test_slots(l[0], l[1], 8);
    }
    test_tie_by_hand();
    test_bytes();
    std::printf("ok\n");
    return 0;
}
