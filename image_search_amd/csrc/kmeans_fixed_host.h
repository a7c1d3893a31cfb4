// kmeans_fixed_host.h — the rules of the fixed-point k-means update without HIP in them: what one component of one member
// adds to its cluster's sum, how a sum becomes a centroid, what the merge of the shards' sums is, and how many rows a
// sharded table may hold for it.  The kernels that implement them: assign_kernels.h ("the same update on exact integer
// sums"); the call that merges across shards: kmeans_sharded.hip.  tests/cpp/test_kmeans_fixed_host.cpp runs this file
// under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace mi {

constexpr int KM_FIXED_BITS = 30;   // a sum counts units of 2^-30

// v = x[r][j] * inv[r] (an fp32 product) -> its integer of 2^-30: rounded to nearest, ties to even (the scaling itself is
// exact); 0 for |v| >= 2, inf and NaN, none of which a member row can produce (a row whose norm is 0, inf or NaN has a NaN
// distance and is no member).  |result| <= 2^31 - 128.
inline int64_t km_fixed_quant(float v) {
    if (!(std::fabs(v) < 2.0f)) return 0;
    return (int64_t)std::nearbyint((double)v * 0x1p30);   // the product is exact in a double; the default rounding mode
}

// fewer than 2^32 members of |q| < 2^31 each: |S| < 2^63
inline bool km_fixed_rows_ok(uint64_t rows) { return rows < (1ull << 32); }

// the sum and the size of a cluster -> one component of its centroid; n == 0: the cluster keeps `previous`
inline float km_fixed_centroid(int64_t S, uint32_t n, float previous) {
    if (n == 0) return previous;
    return (float)((double)S * 0x1p-30 / (double)n);
}

// the merge of one shard's sums and sizes into another's: plain adds, so the shards may arrive in any order
inline void km_fixed_merge(int64_t* S, const int64_t* S_in, size_t n_S, uint32_t* cnt, const uint32_t* cnt_in, size_t n_cnt) {
    for (size_t i = 0; i < n_S; ++i) S[i] += S_in[i];
    for (size_t c = 0; c < n_cnt; ++c) cnt[c] += cnt_in[c];
}

// bytes that cross between shards in one update of S shards: sums and sizes inward from every shard but the first, the
// centroids outward to the same shards
inline uint64_t km_fixed_exchange_bytes(uint32_t S, uint32_t C, uint32_t dim) {
    if (S == 0) return 0;
    return (uint64_t)(S - 1) * C * (8ull * dim + 4) + (uint64_t)(S - 1) * C * dim * 4ull;
}

}  // namespace mi
