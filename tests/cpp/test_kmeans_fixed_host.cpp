// A stand-alone program over image_search_amd/csrc/kmeans_fixed_host.h: the quantisation of the fixed-point k-means sum on
// its edge values, the conversion of a sum to a centroid, the merge of the shards' sums against a sum taken in another order,
// and the row limit.  Built with the address and undefined-behaviour sanitizers by tests/test_kmeans_sharded_host.py; it needs
// neither the library nor a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../image_search_amd/csrc/kmeans_fixed_host.h"

using namespace mi;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static void test_quant() {
    const float u = 0x1p-30f;
    struct { float v; int64_t q; } table[] = {
        {0.0f, 0}, {-0.0f, 0},
        {0.5f * u, 0}, {-0.5f * u, 0},       // ties go to the even neighbour
        {1.5f * u, 2}, {-1.5f * u, -2},
        {2.5f * u, 2}, {-2.5f * u, -2},
        {0.75f * u, 1}, {0.25f * u, 0}, {-0.75f * u, -1},
        {1.0f, 1ll << 30}, {-1.0f, -(1ll << 30)},
        {std::nextafter(2.0f, 0.0f), (1ll << 31) - 128}, {-std::nextafter(2.0f, 0.0f), -((1ll << 31) - 128)},
        {2.0f, 0}, {-2.0f, 0}, {3.0f, 0}, {1e30f, 0},
        {std::numeric_limits<float>::infinity(), 0}, {-std::numeric_limits<float>::infinity(), 0},
        {std::numeric_limits<float>::quiet_NaN(), 0},
        {std::numeric_limits<float>::denorm_min(), 0},
        {0x1p-7f, 1ll << 23}, {0x1p-7f + 0x1p-30f, (1ll << 23) + 1},
    };
    for (const auto& e : table) {
        const int64_t q = km_fixed_quant(e.v);
        if (q != e.q) std::printf("v = %a: got %lld, want %lld\n", (double)e.v, (long long)q, (long long)e.q);
        CHECK(q == e.q);
        CHECK(q < (1ll << 31) && q > -(1ll << 31));
    }
    // every float of a binade around 2^-20: the scaled value has ten fractional bits, the result is its nearest even integer
    for (uint32_t m = 0; m < (1u << 23); m += 4099) {
        const float v = std::ldexp(1.0f + (float)m * 0x1p-23f, -20);
        const double x = (double)v * 0x1p30, f = std::floor(x), r = x - f;
        const int64_t want = (int64_t)f + (r > 0.5 || (r == 0.5 && ((int64_t)f & 1)) ? 1 : 0);
        CHECK(km_fixed_quant(v) == want && km_fixed_quant(-v) == -want);
    }
}

static void test_centroid() {
    CHECK(km_fixed_centroid(0, 0, 7.5f) == 7.5f);                       // an empty cluster keeps its centroid ...
    const float nan = km_fixed_centroid(123, 0, std::numeric_limits<float>::quiet_NaN());
    CHECK(nan != nan);                                                  // ... whatever it holds
    CHECK(km_fixed_centroid(1ll << 30, 1, 0.0f) == 1.0f);
    CHECK(km_fixed_centroid(-(3ll << 30), 4, 0.0f) == -0.75f);
    CHECK(km_fixed_centroid(1, 3, 0.0f) == (float)(0x1p-30 / 3.0));
    CHECK(km_fixed_centroid(0, 5, 9.0f) == 0.0f);
    // the largest sum the limits allow: 2^32 - 1 members of 2^31 - 128 each
    const int64_t big = (int64_t)((1ull << 32) - 1) * ((1ll << 31) - 128);
    CHECK(big > 0 && km_fixed_centroid(big, 0xFFFFFFFFu, 0.0f) == std::nextafter(2.0f, 0.0f));
    CHECK(km_fixed_centroid(-big, 0xFFFFFFFFu, 0.0f) == -std::nextafter(2.0f, 0.0f));
    CHECK(km_fixed_rows_ok(0) && km_fixed_rows_ok((1ull << 32) - 1) && !km_fixed_rows_ok(1ull << 32));
}

static void test_merge() {
    // rows dealt to shards block-cyclically, summed per shard and merged in two orders == summed in row order
    std::mt19937 rng(5);
    std::normal_distribution<float> nd(0.0f, 0.4f);
    const size_t rows = 3000, dim = 24, C = 5, shards = 4, block = 64;
    std::vector<float> v(rows * dim);
    std::vector<uint32_t> label(rows);
    for (float& x : v) x = nd(rng);
    for (uint32_t& l : label) l = rng() % (C + 1);   // C: no member
    std::vector<int64_t> whole(C * dim, 0);
    std::vector<uint32_t> n_whole(C, 0);
    std::vector<std::vector<int64_t>> S(shards, std::vector<int64_t>(C * dim, 0));
    std::vector<std::vector<uint32_t>> n(shards, std::vector<uint32_t>(C, 0));
    for (size_t r = 0; r < rows; ++r) {
        if (label[r] >= C) continue;
        const size_t s = (r / block) % shards;
        ++n_whole[label[r]];
        ++n[s][label[r]];
        for (size_t j = 0; j < dim; ++j) {
            const int64_t q = km_fixed_quant(v[r * dim + j]);
            whole[label[r] * dim + j] += q;
            S[s][label[r] * dim + j] += q;
        }
    }
    std::vector<int64_t> up = S[0], down = S[3];
    std::vector<uint32_t> n_up = n[0], n_down = n[3];
    for (size_t s = 1; s < shards; ++s) km_fixed_merge(up.data(), S[s].data(), C * dim, n_up.data(), n[s].data(), C);
    for (size_t s = 3; s-- > 0;) km_fixed_merge(down.data(), S[s].data(), C * dim, n_down.data(), n[s].data(), C);
    CHECK(up == whole && down == whole && n_up == n_whole && n_down == n_whole);
    for (size_t i = 0; i < C * dim; ++i)
        CHECK(km_fixed_centroid(up[i], n_up[i / dim], 0.0f) == km_fixed_centroid(whole[i], n_whole[i / dim], 0.0f));
    CHECK(km_fixed_exchange_bytes(1, 64, 768) == 0);
    CHECK(km_fixed_exchange_bytes(3, 64, 768) == 2ull * 64 * (8 * 768 + 4) + 2ull * 64 * 768 * 4);
}

int main() {
    test_quant();
    test_centroid();
    test_merge();
    std::printf("ok\n");
    return 0;
}
