// kmeans_seed_sharded_host.h — the plan of mi_knn_sharded_kmeans_seed without HIP in it: how the candidates of a k-means++
// seeding over a block-cyclic table are dealt to the shards, cut into chunks and put back into the table's global order; the
// word a pick travels in; the bytes that cross between shards.  The kernels that run the plan: kmeans_seed_sharded_kernels.h;
// the call: kmeans_seed_sharded.hip.  tests/cpp/test_kmeans_seed_sharded_host.cpp runs this file under the sanitizers.
//
// Rows are dealt block-cyclically (ids.h), so a block of global rows is one shard's local block and the global candidate
// order is a fixed interleaving of the shards' local blocks.  A chunk is a run of one shard's candidates that stays inside
// one local block: walking the chunks in the order they open while the ids ascend visits every candidate in ascending
// global id, which is the position order of mi_knn_kmeans_seed on one table.
#pragma once
#include <cstdint>
#include <vector>

#include "ids.h"

namespace mi {

constexpr uint32_t KMPP_SHARDED_CHUNK = 256;   // positions of a chunk at most (KMPP_CHUNK of kmeans_seed_kernels.h)

struct KmppChunk { uint32_t first, count; };        // positions [first, first + count) of the shard's candidate list
struct KmppChunkAt { uint32_t shard, chunk; };      // a chunk of the global order: whose, and which of its chunks
struct KmppShardPlan {
    std::vector<uint32_t> rows;                     // the shard's candidates as local rows, ascending
    std::vector<KmppChunk> chunks;                  // none for a shard without candidates
};
struct KmppPlan {
    std::vector<KmppShardPlan> shard;
    std::vector<KmppChunkAt> order;                 // global chunk g -> (shard, local chunk)
};

// ids: the live candidates as global ids, ascending, once each, every one a row of the table
inline KmppPlan kmpp_sharded_plan(uint32_t block, uint32_t n_shards, const std::vector<uint64_t>& ids) {
    KmppPlan plan;
    plan.shard.resize(n_shards);
    uint64_t open_block = ~0ull;   // the global block of the chunk that is open (one shard's: a block is not shared)
    for (const uint64_t id : ids) {
        uint32_t s; uint64_t local;
        cyclic_place(block, n_shards, id, &s, &local);
        KmppShardPlan& x = plan.shard[s];
        const uint64_t b = id / block;
        if (b != open_block || x.chunks.back().count == KMPP_SHARDED_CHUNK) {
            plan.order.push_back({s, (uint32_t)x.chunks.size()});
            x.chunks.push_back({(uint32_t)x.rows.size(), 0u});
            open_block = b;
        }
        x.rows.push_back((uint32_t)local);
        ++x.chunks.back().count;
    }
    return plan;
}

// The word shard 0 sends to every shard per seed (16 bytes): the owner, its chunk, and in rem_mode the remainder of the
// threshold inside that chunk (< 256 * 2^31: bits 0 .. 61) under the mode (bits 62 .. 63).
struct KmppPick { uint32_t shard, chunk; unsigned long long rem_mode; };
constexpr unsigned long long KMPP_PICK_WEIGHTED = 0ull, KMPP_PICK_FALLBACK = 1ull, KMPP_PICK_TOTAL = 2ull;
constexpr int KMPP_PICK_MODE_SHIFT = 62;

// what a shard answers a pick with: {global id, 1 = this shard owns the pick} and the row's fp32 values
inline uint32_t kmpp_slot_words(uint32_t dim) { return 2u + dim / 2u; }   // in 64-bit words (dim is even)

// Bytes copied between shards by one call of S shards, C seeds: before each of the C + 1 picks (the last one only takes the
// total) every shard but the first sends its lowest-unpicked word and its chunk sums, 8 * (1 + chunks) bytes; per seed the
// first shard sends the 16-byte pick word to, receives a slot of 16 + 4 dim bytes from, and sends the 4 dim bytes of the
// chosen row to every other shard.  chunks_elsewhere = the chunks of shards 1 .. S - 1.  Copies within the first shard are
// not counted.
inline uint64_t kmpp_sharded_exchange_bytes(uint32_t S, uint64_t chunks_elsewhere, uint32_t C, uint32_t dim) {
    if (S <= 1) return 0;
    return ((uint64_t)C + 1) * 8ull * (chunks_elsewhere + (S - 1)) + (uint64_t)C * (S - 1) * (32ull + 8ull * dim);
}

}  // namespace mi
