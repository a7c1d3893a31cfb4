// The host-only pieces of mi_knn_search_compound (image_search_amd/csrc/compound_host.h) as a stand-alone program: the
// argument rules, the padding of the term set, the dim and grid rules (scan_call.h's), the record's layout and the copy into caller arrays of exactly
// k and k x T elements.  Built with -fsanitize=address,undefined (tests/test_compound_host.py) every array is heap memory of
// its exact size, so a read or write one element too far is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../image_search_amd/csrc/compound_host.h"
#include "../../image_search_amd/csrc/scan_call.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    const float v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w_ok[3] = {0.0f, 0.5f, INFINITY}, w_nan[2] = {0.1f, NAN}, w_neg[1] = {-1e-9f};
    const uint64_t ids[1] = {0};
    auto chk = [&](const void* tt, const float* pos, uint32_t n_pos, int mode, const float* neg, const float* within, uint32_t n_neg, uint32_t k,
                   const void* among, uint64_t n_among, const void* idx, const void* dist) {
        return compound_check_args(tt, pos, n_pos, mode, neg, within, n_neg, k, among, n_among, idx, dist, &why);
    };
    EXPECT(chk(&t, v, 1, MI_COMPOUND_ALL, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 5, MI_COMPOUND_ANY, v, w_ok, 3, 4096, ids, 1, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 8, MI_COMPOUND_ANY, nullptr, nullptr, 0, 64, ids, 0, &o, &o) == MI_OK);
    EXPECT(chk(nullptr, v, 1, 0, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, nullptr, 1, 0, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, nullptr, nullptr, 0, 1, nullptr, 0, nullptr, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, nullptr, nullptr, 0, 1, nullptr, 0, &o, nullptr) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 0, 0, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, nullptr, nullptr, 0, 0, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 0, 0, nullptr, nullptr, 0, 5000, nullptr, 0, &o, &o) == MI_ERR_INVALID);   // zero before "too large"
    EXPECT(chk(&t, v, 1, 2, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, -1, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, nullptr, w_ok, 1, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, v, nullptr, 1, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, nullptr, nullptr, 0, 1, nullptr, 3, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, v, w_nan, 2, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, v, w_neg, 1, 1, nullptr, 0, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 9, 0, nullptr, nullptr, 0, 1, nullptr, 0, &o, &o) == MI_ERR_UNSUPPORTED);
    EXPECT(chk(&t, v, 6, 0, v, w_ok, 3, 1, nullptr, 0, &o, &o) == MI_ERR_UNSUPPORTED);
    EXPECT(chk(&t, v, 1, 0, v, w_neg, 0xFFFFFFFFu, 1, nullptr, 0, &o, &o) == MI_ERR_UNSUPPORTED);   // the count is judged before a threshold is read
    EXPECT(chk(&t, v, 1, 0, nullptr, nullptr, 0, 4097, nullptr, 0, &o, &o) == MI_ERR_UNSUPPORTED);
    EXPECT(why && why[0] != '\0');
    for (uint32_t dim : {128u, 256u, 512u, 768u, 1024u}) EXPECT(scan_dim_ok(dim));
    for (uint32_t dim : {0u, 64u, 192u, 384u, 2048u}) EXPECT(!scan_dim_ok(dim));
}

static void term_set(uint32_t n_pos, uint32_t n_neg, uint32_t dim) {
    std::vector<float> pos((size_t)n_pos * dim), neg((size_t)n_neg * dim), within(n_neg);
    for (size_t j = 0; j < pos.size(); ++j) pos[j] = 1.0f + (float)j;
    for (size_t j = 0; j < neg.size(); ++j) neg[j] = -1.0f - (float)j;
    for (uint32_t j = 0; j < n_neg; ++j) within[j] = 0.25f * (float)(j + 1);
    const CompoundSet c = compound_set(pos.data(), n_pos, n_neg ? neg.data() : nullptr, n_neg ? within.data() : nullptr, n_neg, dim);
    const uint32_t T = n_pos + n_neg;
    EXPECT(c.T == T && c.padded >= T && (c.padded == 2 || c.padded == 4 || c.padded == 8) && (c.padded == 2 || c.padded / 2 < T));
    EXPECT(c.terms.size() == (size_t)c.padded * dim);
    for (uint32_t u = 0; u < c.padded; ++u) {
        const bool is_neg = u >= n_pos && u < T;
        EXPECT(((c.neg_mask >> u) & 1u) == (is_neg ? 1u : 0u));
        EXPECT(c.within[u] == (is_neg ? within[u - n_pos] : 0.0f));
        const float* want = u < n_pos ? pos.data() + (size_t)u * dim : is_neg ? neg.data() + (size_t)(u - n_pos) * dim : pos.data();
        for (uint32_t e = 0; e < dim; ++e) EXPECT(c.terms[(size_t)u * dim + e] == want[e]);
    }
    EXPECT((c.neg_mask >> c.padded) == 0);
}

static uint32_t compound_grid(uint64_t n, int n_cu, int option) { return scan_grid(n, n_cu, option, COMPOUND_BLOCKS_PER_CU); }

static void grid() {
    EXPECT(compound_grid(1, 256, 0) == 1 && compound_grid(64, 256, 0) == 1 && compound_grid(257, 256, 0) == 2);
    EXPECT(compound_grid(5000, 256, 0) == 20);            // 79 tiles: 80 per-wave lists, the two-level merge
    EXPECT(compound_grid(1000, 256, 0) == 4 && compound_grid(1000, 256, 1) == 1 && compound_grid(1000, 256, 3) == 3 && compound_grid(1000, 256, 9) == 4);
    EXPECT(compound_grid(10000000ull, 256, 0) == 512 && compound_grid(10000000ull, 256, 4096) == 4096);
    EXPECT(compound_grid(0xFFFFFFFFull, 256, 0x7FFFFFFF) == 16777216u);
}

static void record(uint32_t k, uint32_t T, bool with_term_dist) {
    const CompoundRecord r = compound_record(k, T);
    EXPECT(r.idx == 0 && r.stats % 8 == 0 && r.dist % 4 == 0 && r.term_dist % 4 == 0);
    EXPECT(r.stats == (size_t)k * 8 && r.dist == r.stats + 32 && r.term_dist == r.dist + (size_t)k * 4 && r.bytes == r.term_dist + (size_t)k * T * 4);
    std::vector<unsigned char> rec(r.bytes);
    for (uint32_t j = 0; j < k; ++j) {
        const uint64_t id = 1000 + j;
        const float d = 0.5f + (float)j;
        std::memcpy(rec.data() + r.idx + (size_t)j * 8, &id, 8);
        std::memcpy(rec.data() + r.dist + (size_t)j * 4, &d, 4);
        for (uint32_t u = 0; u < T; ++u) {
            const float td = (float)(j * 10 + u);
            std::memcpy(rec.data() + r.term_dist + ((size_t)j * T + u) * 4, &td, 4);
        }
    }
    const uint64_t st_in[4] = {11, 22, 33, 44};
    std::memcpy(rec.data() + r.stats, st_in, 32);
    std::vector<uint64_t> idx(k);
    std::vector<float> dist(k), td(with_term_dist ? (size_t)k * T : 0);
    uint64_t st[4] = {0, 0, 0, 0};
    compound_unpack(rec.data(), k, T, idx.data(), dist.data(), with_term_dist ? td.data() : nullptr, st);
    EXPECT(st[0] == 11 && st[1] == 22 && st[2] == 33 && st[3] == 44);
    for (uint32_t j = 0; j < k; ++j) {
        EXPECT(idx[j] == 1000 + j && dist[j] == 0.5f + (float)j);
        if (with_term_dist)
            for (uint32_t u = 0; u < T; ++u) EXPECT(td[(size_t)j * T + u] == (float)(j * 10 + u));
    }
    compound_pad(k, T, idx.data(), dist.data(), with_term_dist ? td.data() : nullptr);
    for (uint32_t j = 0; j < k; ++j) EXPECT(idx[j] == MI_KNN_NO_ID && std::isinf(dist[j]) && dist[j] > 0);
    for (float v : td) EXPECT(std::isinf(v) && v > 0);
}

int main() {
    args();
    for (uint32_t n_pos = 1; n_pos <= 8; ++n_pos)
        for (uint32_t n_neg = 0; n_pos + n_neg <= 8; ++n_neg) term_set(n_pos, n_neg, n_pos % 2 ? 128 : 768);
    grid();
    for (uint32_t k : {1u, 10u, 64u, 65u, 4096u})
        for (uint32_t T : {1u, 3u, 8u}) { record(k, T, true); record(k, T, false); }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
