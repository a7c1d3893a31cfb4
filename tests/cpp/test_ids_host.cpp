// The id space of a table (image_search_amd/csrc/ids.h) as a stand-alone program: local row <-> id for plain tables and for
// shards of a block-cyclic table (every row's id maps back, the ids between and around them do not), and the placement
// arithmetic of the block-cyclic table against a brute-force placement of every row: place, id_of_local and local_of_id agree,
// no other shard claims a row, the rows-of-shard rule counts what was placed, and at `after + 1` it is the number of a shard's
// rows at or below a cursor.  Built with -fsanitize=address,undefined (tests/test_ids_host.py); every array is heap memory of
// its exact size.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../image_search_amd/csrc/ids.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

// id of a local row, written out: what id_of_local must give
static uint64_t id_of(const IdMap& m, uint64_t local) {
    if (m.n <= 1 || m.block == 0) return m.base + local;
    return m.base + ((local / m.block) * m.n + m.rank) * m.block + local % m.block;
}

static void one_table(const IdMap& m, uint64_t rows) {
    // every row's id maps back; the ids between the rows' and the ids around the range do not
    std::vector<char> held(rows * std::max(m.n, 1u) + 2 * (m.block ? m.block : 1) + 4, 0);
    for (uint64_t l = 0; l < rows; ++l) {
        uint64_t back = ~0ull;
        EXPECT(id_of_local(m, l) == id_of(m, l));
        EXPECT(local_of_id(m, rows, id_of(m, l), &back) && back == l);
        held[id_of(m, l) - m.base] = 1;
    }
    for (uint64_t off = 0; off < held.size(); ++off) {
        uint64_t l = 0;
        EXPECT(local_of_id(m, rows, m.base + off, &l) == (held[off] != 0));
    }
    uint64_t l = 0;
    if (m.base) EXPECT(!local_of_id(m, rows, m.base - 1, &l));
}

static void last_row_of_2_32() {
    const IdMap m{0, 0, 0, 0};
    uint64_t l = 0;
    EXPECT(local_of_id(m, 0x100000000ull, 0xFFFFFFFFull, &l) && l == 0xFFFFFFFFull);
    EXPECT(!local_of_id(m, 0x100000000ull, 0x100000000ull, &l));
    EXPECT(id_of_local(m, 0xFFFFFFFFull) == 0xFFFFFFFFull);
}

// every global row of a table of `total` rows placed by brute force, against the arithmetic
static void placement(uint32_t block, uint32_t n, uint64_t total) {
    std::vector<uint64_t> held(n, 0);     // per shard: rows placed so far = local rows with global row <= r
    std::vector<IdMap> maps;
    for (uint32_t s = 0; s < n; ++s) maps.push_back(IdMap{0, block, n, s});
    for (uint32_t s = 0; s < n; ++s) EXPECT(cyclic_rows_of(block, n, s, 0) == 0);
    for (uint64_t r = 0; r < total; ++r) {
        uint32_t s = ~0u;
        uint64_t local = ~0ull;
        cyclic_place(block, n, r, &s, &local);
        EXPECT(s < n);
        if (s >= n) return;
        EXPECT(local == held[s]);         // a shard's local rows ascend with their global ids
        ++held[s];
        EXPECT(id_of_local(maps[s], local) == r);
        for (uint32_t u = 0; u < n; ++u) {
            // (a shard is asked about the rows it holds once the whole table is there)
            uint64_t back = ~0ull;
            const bool mine = local_of_id(maps[u], cyclic_rows_of(block, n, u, total), r, &back);
            EXPECT(mine == (u == s));
            if (u == s) EXPECT(back == local);
            // the rows u holds of a table of r + 1 rows = its rows at or below r, by count
            EXPECT(cyclic_rows_of(block, n, u, r + 1) == held[u]);
        }
    }
    uint64_t sum = 0;
    for (uint32_t s = 0; s < n; ++s) {
        EXPECT(cyclic_rows_of(block, n, s, total) == held[s]);
        sum += held[s];
    }
    EXPECT(sum == total);
}

int main() {
    one_table(IdMap{0, 0, 0, 0}, 300);
    one_table(IdMap{1ull << 33, 0, 0, 0}, 130);
    one_table(IdMap{0, 0, 0, 0}, 0);
    for (uint32_t rank = 0; rank < 3; ++rank) one_table(IdMap{0, 16, 3, rank}, 100);   // a shard with a ragged last block
    one_table(IdMap{1000, 64, 2, 1}, 64);
    last_row_of_2_32();
    for (uint32_t block : {1u, 8u, 64u})
        for (uint32_t n : {1u, 2u, 3u, 8u})
            for (uint64_t total = 0; total <= 300; ++total) placement(block, n, total);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
