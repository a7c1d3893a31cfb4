// A stand-alone program over image_search_amd/csrc/kmeans_seed_sharded_host.h: the plan of the k-means++ seeding across
// shards — the candidates dealt to the shards as local rows, the chunks, the global order of the chunks — on five layouts,
// over all rows and over subsets with gaps of whole blocks, with empty shards; and the closed form of the bytes exchanged.
// Built with the address and undefined-behaviour sanitizers by tests/test_kmeans_seed_sharded_host.py; it needs neither the
// library nor a GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../image_search_amd/csrc/kmeans_seed_sharded_host.h"

using namespace mi;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// every rule of the plan, for the candidates `ids` (ascending, unique) of a table dealt as (shards, block)
static void check_plan(uint32_t shards, uint32_t block, const std::vector<uint64_t>& ids) {
    const KmppPlan plan = kmpp_sharded_plan(block, shards, ids);
    CHECK(plan.shard.size() == shards);
    size_t n_rows = 0, n_chunks = 0;
    for (uint32_t s = 0; s < shards; ++s) {
        const KmppShardPlan& x = plan.shard[s];
        n_rows += x.rows.size();
        n_chunks += x.chunks.size();
        CHECK(std::is_sorted(x.rows.begin(), x.rows.end()));
        CHECK(std::adjacent_find(x.rows.begin(), x.rows.end()) == x.rows.end());
        CHECK(x.rows.empty() == x.chunks.empty());
        uint32_t at = 0;   // the chunks tile the shard's list in order
        for (const KmppChunk& c : x.chunks) {
            CHECK(c.first == at && c.count >= 1 && c.count <= KMPP_SHARDED_CHUNK);
            CHECK(x.rows[c.first] / block == x.rows[c.first + c.count - 1] / block);   // inside one local block
            at += c.count;
        }
        CHECK(at == x.rows.size());
    }
    CHECK(n_rows == ids.size() && n_chunks == plan.order.size());
    // the chunks in global order concatenate to the sorted candidates, and every chunk is visited once
    std::vector<uint64_t> walked;
    std::vector<std::vector<char>> seen(shards);
    for (uint32_t s = 0; s < shards; ++s) seen[s].assign(plan.shard[s].chunks.size(), 0);
    for (const KmppChunkAt& g : plan.order) {
        CHECK(g.shard < shards && g.chunk < plan.shard[g.shard].chunks.size());
        CHECK(!seen[g.shard][g.chunk]);
        seen[g.shard][g.chunk] = 1;
        const KmppChunk& c = plan.shard[g.shard].chunks[g.chunk];
        const IdMap map{0, block, shards, g.shard};
        for (uint32_t k = 0; k < c.count; ++k) {
            const uint64_t id = shards > 1 ? id_of_local(map, plan.shard[g.shard].rows[c.first + k]) : plan.shard[g.shard].rows[c.first + k];
            uint32_t s; uint64_t local;
            cyclic_place(block, shards, id, &s, &local);
            CHECK(s == g.shard && local == plan.shard[g.shard].rows[c.first + k]);
            walked.push_back(id);
        }
    }
    CHECK(walked == ids);
}

static std::vector<uint64_t> all_rows(uint64_t n) {
    std::vector<uint64_t> ids(n);
    for (uint64_t r = 0; r < n; ++r) ids[r] = r;
    return ids;
}

int main() {
    const struct { uint32_t shards, block; } layouts[] = {{1, 4096}, {3, 64}, {2, 128}, {4, 64}, {2, 960}};
    std::mt19937 rng(11);
    for (const auto& l : layouts) {
        for (uint64_t n : {1ull, 63ull, 100ull, 3001ull, 8193ull}) {
            check_plan(l.shards, l.block, all_rows(n));
            // a subset: whole blocks left out (a shard may lose every block), single rows left out of the others
            std::vector<uint64_t> some;
            for (uint64_t r = 0; r < n; ++r) {
                const uint64_t b = r / l.block;
                if (b % 5 == 1 || b % 7 == 3) continue;
                if (rng() % 4 == 0) continue;
                some.push_back(r);
            }
            check_plan(l.shards, l.block, some);
            // one shard's blocks only: every other shard takes part with zero chunks
            std::vector<uint64_t> one;
            for (uint64_t r = 0; r < n; ++r)
                if ((r / l.block) % l.shards == l.shards - 1) one.push_back(r);
            check_plan(l.shards, l.block, one);
            const KmppPlan p = kmpp_sharded_plan(l.block, l.shards, one);
            for (uint32_t s = 0; s + 1 < l.shards; ++s) CHECK(p.shard[s].rows.empty() && p.shard[s].chunks.empty());
        }
        check_plan(l.shards, l.block, {});
    }
    // 100 rows on (4, 64): shards 2 and 3 hold no rows
    {
        const KmppPlan p = kmpp_sharded_plan(64, 4, all_rows(100));
        CHECK(p.shard[0].rows.size() == 64 && p.shard[1].rows.size() == 36 && p.shard[2].rows.empty() && p.shard[3].rows.empty());
        CHECK(p.order.size() == 2 && p.order[0].shard == 0 && p.order[1].shard == 1);
    }
    // a block longer than a chunk is cut at 256 positions: (2, 960) holds 960 = 3 * 256 + 192 per block
    {
        const KmppPlan p = kmpp_sharded_plan(960, 2, all_rows(2000));
        CHECK(p.shard[0].chunks.size() == 4 + 1 && p.shard[1].chunks.size() == 4);
        CHECK(p.shard[0].chunks[3].count == 192 && p.shard[0].chunks[4].count == 80 && p.shard[0].chunks[4].first == 960);
        CHECK(p.order[4].shard == 1 && p.order[4].chunk == 0 && p.order[8].shard == 0 && p.order[8].chunk == 4);
    }
    // the bytes exchanged: nothing with one shard; otherwise the words before each of the C + 1 picks and, per seed and
    // other shard, the pick word (16), the slot (16 + 4 dim) and the centre (4 dim)
    CHECK(sizeof(KmppPick) == 16);
    CHECK(kmpp_slot_words(768) * 8 == 16 + 4 * 768);
    CHECK(kmpp_sharded_exchange_bytes(1, 0, 64, 768) == 0);
    CHECK(kmpp_sharded_exchange_bytes(0, 0, 64, 768) == 0);
    CHECK(kmpp_sharded_exchange_bytes(3, 31, 16, 768) == 17ull * 8 * (31 + 2) + 16ull * 2 * (16 + (16 + 4 * 768) + 4 * 768));
    CHECK(kmpp_sharded_exchange_bytes(4, 0, 1, 128) == 2ull * 8 * 3 + 3ull * (32 + 8 * 128));
    CHECK(kmpp_sharded_exchange_bytes(8, 1ull << 24, 65536, 1024) ==
          65537ull * 8 * ((1ull << 24) + 7) + 65536ull * 7 * (32 + 8 * 1024));
    std::printf("ok\n");
    return 0;
}
