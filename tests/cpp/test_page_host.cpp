// The host-only pieces of mi_knn_search_page (image_search_amd/csrc/page_host.h) as a stand-alone program: the argument rules
// in the contract's order, the key transform, the cursor -> first_key rule for a plain table, for a shard of a block-cyclic
// table and for the sharded call (against a brute-force placement of every row), the `hi` rule, the grid rule (scan_call.h's,
// at the paged search's factor), the record's layout and the copy into caller arrays of exactly k elements.  Built with -fsanitize=address,undefined
// (tests/test_page_host.py) every array is heap memory of its exact size, so a read or write one element too far is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../image_search_amd/csrc/page_host.h"
#include "../../image_search_amd/csrc/scan_call.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static const uint64_t NO = MI_KNN_NO_ID;

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    const float v[4] = {0, 0, 0, 0};
    const uint64_t ids[1] = {0};
    auto chk = [&](const void* tt, const float* q, uint32_t k, float ad, uint64_t ai, float md, const void* among, uint64_t n_among,
                   const void* idx, const void* dist) { return page_check_args(tt, q, k, ad, ai, md, among, n_among, idx, dist, &why); };
    EXPECT(chk(&t, v, 1, 0.0f, NO, INFINITY, nullptr, 0, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 4096, 0.25f, 7, 0.5f, ids, 1, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 64, -0.0f, 0, -INFINITY, ids, 0, &o, &o) == MI_OK);          // an empty set; a bound below everything
    EXPECT(chk(&t, v, 10, NAN, NO, INFINITY, nullptr, 0, &o, &o) == MI_OK);         // after_dist is ignored without a cursor
    EXPECT(chk(&t, v, 10, INFINITY, 3, INFINITY, nullptr, 0, &o, &o) == MI_OK);
    EXPECT(chk(nullptr, v, 1, 0.0f, NO, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, nullptr, 1, 0.0f, NO, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0.0f, NO, INFINITY, nullptr, 0, nullptr, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0.0f, NO, INFINITY, nullptr, 0, &o, nullptr) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0.0f, NO, INFINITY, nullptr, 3, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, NAN, 5, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0.0f, NO, NAN, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 0, 0.0f, NO, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 4097, 0.0f, NO, INFINITY, nullptr, 0, &o, &o) == MI_ERR_UNSUPPORTED);
    EXPECT(chk(&t, v, 4097, NAN, 5, INFINITY, nullptr, 0, &o, &o) == MI_ERR_INVALID);     // the cursor and the bound are judged before k
    EXPECT(chk(&t, v, 4097, 0.0f, NO, NAN, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(why && why[0] != '\0');
}

static void keys() {
    const float d[] = {-INFINITY, -1.5f, -0.0f, 0.0f, 1e-45f, 0.25f, 2.0f, INFINITY, NAN};
    for (size_t j = 0; j + 1 < sizeof d / sizeof d[0]; ++j) EXPECT(page_dist_key(d[j]) < page_dist_key(d[j + 1]));
    EXPECT(page_dist_key(NAN) == 0xFFFFFFFFu && page_dist_key(-NAN) == 0xFFFFFFFFu);
    EXPECT(page_dist_key(-0.0f) == 0x7FFFFFFFu && page_dist_key(0.0f) == 0x80000000u && page_dist_key(INFINITY) == 0xFF800000u);
    // hi: every row part of the bound's distance, nothing of the next
    EXPECT(page_hi(0.0f) == 0x80000000FFFFFFFFull && page_hi(-0.0f) == 0x7FFFFFFFFFFFFFFFull && page_hi(INFINITY) == 0xFF800000FFFFFFFFull);
    EXPECT(page_hi(INFINITY) < ((uint64_t)page_dist_key(NAN) << 32));     // a NaN distance is above every bound
    EXPECT(page_hi(0.25f) + 1 == ((uint64_t)page_dist_key(std::nextafterf(0.25f, 1.0f)) << 32));
}

// (the id space itself — id <-> local row, the placement arithmetic — is tests/cpp/test_ids_host.cpp's)
static void cursor_one_table(const IdMap& m, uint64_t rows) {
    // a cursor at every row's id; none at the ids between the rows' and around the range
    std::vector<char> held(rows * std::max(m.n, 1u) + 2 * (m.block ? m.block : 1) + 4, 0);
    for (uint64_t l = 0; l < rows; ++l) {
        held[id_of_local(m, l) - m.base] = 1;
        uint64_t fk = 1;
        EXPECT(page_first_key(m, rows, 0.25f, id_of_local(m, l), &fk));
        EXPECT(fk == (((uint64_t)page_dist_key(0.25f) << 32) | l) + 1);          // the cursor key + 1
    }
    for (uint64_t off = 0; off < held.size(); ++off) {
        uint64_t fk = 1;
        EXPECT(page_first_key(m, rows, 0.5f, m.base + off, &fk) == (held[off] != 0));
    }
    uint64_t fk = 1;
    if (m.base) EXPECT(!page_first_key(m, rows, 0.5f, m.base - 1, &fk));
    EXPECT(page_first_key(m, rows, NAN, NO, &fk) && fk == 0);                     // no cursor: from the start, after_dist ignored
    // -0 and +0 are different cursors
    if (rows) {
        uint64_t a = 0, b = 0;
        EXPECT(page_first_key(m, rows, -0.0f, id_of_local(m, 0), &a) && page_first_key(m, rows, 0.0f, id_of_local(m, 0), &b) &&
               a + (1ull << 32) == b);
    }
}

static void first_key_carry() {
    // the last possible row of a distance: + 1 carries into the distance word, i.e. "nothing of that distance is left"
    const IdMap m{0, 0, 0, 0};
    uint64_t fk = 0;
    EXPECT(page_first_key(m, 0x100000000ull, 0.25f, 0xFFFFFFFFull, &fk) && fk == ((uint64_t)(page_dist_key(0.25f) + 1) << 32));
    EXPECT(page_first_key_at(INFINITY, 0x100000000ull) == 0xFF80000100000000ull);   // the largest cursor does not wrap
    EXPECT(page_first_key_at(-INFINITY, 0) == ((uint64_t)page_dist_key(-INFINITY) << 32));
}

// global row r of a block-cyclic table: shard and local row (mi_knn_sharded_place)
static void place(uint32_t block, uint32_t n, uint64_t r, uint32_t* s, uint64_t* local) {
    const uint64_t blk = r / block;
    *s = (uint32_t)(blk % n);
    *local = (blk / n) * block + r % block;
}

static void cursor_sharded(uint32_t block, uint32_t n, uint64_t rows) {
    std::vector<uint64_t> below(n, 0);    // per shard: local rows with global row <= after, by brute force
    for (uint64_t after = 0; after < rows; ++after) {
        uint32_t s; uint64_t local;
        place(block, n, after, &s, &local);
        EXPECT(local == below[s]);        // a shard's local rows ascend with their global ids
        ++below[s];
        for (uint32_t u = 0; u < n; ++u) {
            EXPECT(cyclic_rows_of(block, n, u, after + 1) == below[u]);
            // the shard that holds the cursor's row gets what the one-table rule gives it
            if (u == s) {
                const IdMap m{0, block, n, u};
                uint64_t fk = 0;
                EXPECT(page_first_key(m, rows, 0.125f, after, &fk) && fk == page_first_key_at(0.125f, below[u]));
            }
        }
    }
}

static uint32_t page_grid(uint64_t n, int n_cu, int option) { return scan_grid(n, n_cu, option, PAGE_BLOCKS_PER_CU); }

static void grid() {
    EXPECT(page_grid(1, 256, 0) == 1 && page_grid(64, 256, 0) == 1 && page_grid(257, 256, 0) == 2);
    EXPECT(page_grid(5000, 256, 0) == 20);            // 79 tiles: 80 per-wave lists, the two-level merge
    EXPECT(page_grid(1000, 256, 0) == 4 && page_grid(1000, 256, 1) == 1 && page_grid(1000, 256, 3) == 3 && page_grid(1000, 256, 1000) == 4);
    EXPECT(page_grid(10000000ull, 256, 0) == 1024 && page_grid(10000000ull, 256, 4096) == 4096);
    EXPECT(page_grid(0xFFFFFFFFull, 256, 0x7FFFFFFF) == 16777216u && page_grid(1000, 0, 0) == 4);
}

static void record(uint32_t k, bool with_counts) {
    const PageRecord r = page_record(k);
    EXPECT(r.idx == 0 && r.counts == (size_t)k * 8 && r.dist == r.counts + 32 && r.bytes == r.dist + (size_t)k * 4);
    std::vector<unsigned char> rec(r.bytes);
    for (uint32_t j = 0; j < k; ++j) {
        const uint64_t id = (1ull << 33) + j;
        const float d = 0.5f + (float)j;
        std::memcpy(rec.data() + r.idx + (size_t)j * 8, &id, 8);
        std::memcpy(rec.data() + r.dist + (size_t)j * 4, &d, 4);
    }
    const uint64_t c_in[4] = {11, 22, 33, 44};
    std::memcpy(rec.data() + r.counts, c_in, 32);
    std::vector<uint64_t> idx(k), counts(with_counts ? 4 : 0);
    std::vector<float> dist(k);
    page_unpack(rec.data(), k, idx.data(), dist.data(), with_counts ? counts.data() : nullptr);
    for (uint32_t j = 0; j < k; ++j) EXPECT(idx[j] == (1ull << 33) + j && dist[j] == 0.5f + (float)j);
    if (with_counts) EXPECT(counts[0] == 11 && counts[1] == 22 && counts[2] == 33 && counts[3] == 44);
    page_pad(k, idx.data(), dist.data(), with_counts ? counts.data() : nullptr);
    for (uint32_t j = 0; j < k; ++j) EXPECT(idx[j] == MI_KNN_NO_ID && std::isinf(dist[j]) && dist[j] > 0);
    for (uint64_t c : counts) EXPECT(c == 0);
}

int main() {
    args();
    keys();
    cursor_one_table(IdMap{0, 0, 0, 0}, 300);
    cursor_one_table(IdMap{1ull << 33, 0, 0, 0}, 130);
    cursor_one_table(IdMap{0, 0, 0, 0}, 0);
    for (uint32_t rank = 0; rank < 3; ++rank) cursor_one_table(IdMap{0, 16, 3, rank}, 100);   // a shard with a ragged last block
    cursor_one_table(IdMap{1000, 64, 2, 1}, 64);
    first_key_carry();
    cursor_sharded(16, 2, 200);
    cursor_sharded(64, 3, 1000);
    cursor_sharded(1, 4, 37);
    cursor_sharded(50, 1, 120);
    grid();
    for (uint32_t k : {1u, 10u, 64u, 65u, 4096u}) { record(k, true); record(k, false); }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
