// kmeans_seed_sharded_kernels.h — device code of mi_knn_sharded_kmeans_seed: the k-means++ seeding of kmeans_seed_kernels.h
// over a block-cyclic table.  Per candidate position a shard keeps what the single table keeps (D, w, the two flag bits); a
// pass leaves one uint64 sum of w per chunk of the plan (kmeans_seed_sharded_host.h).  The first shard scans every shard's
// chunk sums in the table's global order, turns z into the threshold and names the owner and its chunk in a 16-byte word;
// the owner finds the position inside its chunk and hands the row out; the first shard appends it and writes the centre every
// shard's next pass reads.  The distance block is the written-out block of kmpp_pass_kernel, copied and not shared (DESIGN.md
// 5.19), the weights are integers and a prefix sum of integers is the same in any order: every pick equals the single
// table's.  No atomics; no kernel waits for or polls another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ids.h"
#include "kmeans_seed_sharded_host.h"   // KmppChunk, KmppChunkAt, KmppPick
#include "knn_shared.h"

namespace mi {

// (kmeans_seed_kernels.h defines kernels that are no templates: a second translation unit cannot include it.  What this
// file needs of it — the flag bits and the scan of one workgroup — is restated here.)
constexpr uint32_t KMPP_USABLE = 1u, KMPP_PICKED = 2u;
constexpr uint32_t KMPP_NO_POS = 0xFFFFFFFFu;
static_assert(KMPP_SHARDED_CHUNK % 16 == 0 && KMPP_SHARDED_CHUNK <= 256, "a chunk: 16-lane groups, one locate workgroup");
static_assert(sizeof(KmppPick) == 16, "the pick word is 16 bytes");

// One workgroup of 1024 threads over n values val(0 .. n - 1): thread t sums a contiguous piece, the pieces are scanned in
// LDS.  Returns the total; lo / hi = the thread's piece, excl = the sum of everything before it, incl = excl + its own.
template <class F>
__device__ __forceinline__ unsigned long long kmpp_sharded_scan(F val, uint32_t n, unsigned long long* sc, uint32_t& lo, uint32_t& hi,
                                                                unsigned long long& excl, unsigned long long& incl) {
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint64_t l = (uint64_t)t * per, h = l + per;
    lo = (uint32_t)(l < n ? l : n);
    hi = (uint32_t)(h < n ? h : n);
    unsigned long long own = 0ull;
    for (uint32_t k = lo; k < hi; ++k) own += val(k);
    sc[t] = own;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const unsigned long long v = t >= off ? sc[t - off] : 0ull;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    incl = sc[t];
    excl = incl - own;
    return sc[1023];
}

// Workgroup b owns the chunk desc[b] (1 .. 256 positions of `list`), a 16-lane group one position per step.  FIRST: the
// pass before pick 0 — the row against itself decides "usable", D = unset, w = usable.  Otherwise the centre is the [DIM]
// fp32 row at `centre`, on this shard's device.
template <int NCH, bool FIRST = false>
__global__ __launch_bounds__(256) void kmpp_sharded_pass_kernel(const float* __restrict__ table, const uint32_t* __restrict__ list,
                                                                const KmppChunk* __restrict__ desc, const float* __restrict__ centre,
                                                                float* __restrict__ D, uint32_t* __restrict__ w,
                                                                uint32_t* __restrict__ flags, unsigned long long* __restrict__ chunk_sum) {
    constexpr int DIM = NCH * 64;
    __shared__ unsigned long long part[16];
    const int lane = threadIdx.x & 63, i = lane & 15, g = threadIdx.x >> 4;
    const uint32_t first = desc[blockIdx.x].first, count = desc[blockIdx.x].count;   // count >= 1
    f32x4 qf[NCH];
    float sq = 0.0f;  // sqrt(q.q), same summation order as a row
    if (!FIRST) {
        const f32x4* pa = reinterpret_cast<const f32x4*>(centre) + i;
#pragma unroll
        for (int t = 0; t < NCH; ++t) qf[t] = pa[16 * t];
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
        sq = sqrtf(a.sumsq());
    }
    unsigned long long sum = 0ull;
    // (whole waves stay in the loop: row16_sum is a cross-lane operation)
    const uint32_t steps = (count + 15u) & ~15u;
    for (uint32_t o = (uint32_t)g; o < steps; o += 16) {
        const bool live = o < count;
        const uint32_t p = first + (live ? o : count - 1);
        const f32x4* pb = reinterpret_cast<const f32x4*>(table + (uint64_t)list[p] * DIM) + i;
        if (FIRST) {
#pragma unroll
            for (int t = 0; t < NCH; ++t) qf[t] = pb[16 * t];
            RowAcc<NCH> a; a.zero();
#pragma unroll
            for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
            sq = sqrtf(a.sumsq());
        }
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], FIRST ? qf[t] : pb[16 * t]);
        const float d = a.dot(), s = a.sumsq();
        const float dist = 1.0f - d / (sq * sqrtf(s));
        if (live && i == 0) {
            uint32_t wv = 0u;
            if (FIRST) {
                wv = dist == dist ? 1u : 0u;
                flags[p] = wv ? KMPP_USABLE : 0u;
                D[p] = __uint_as_float(0x7FC00000u);
            } else {
                float best = D[p];
                if (dist == dist && !(dist >= best)) {   // (best unset = NaN: the comparison is false)
                    best = dist;
                    D[p] = best;
                }
                if (flags[p] == KMPP_USABLE && best == best) wv = (uint32_t)(fminf(fmaxf(best, 0.0f), 2.0f) * 0x1p30f);
            }
            w[p] = wv;
            sum += wv;
        }
    }
    if (i == 0) part[g] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0ull;
        for (int u = 0; u < 16; ++u) all += part[u];
        chunk_sum[blockIdx.x] = all;
    }
}

// Pick j on the first shard's device (one workgroup of 1024).  all = every shard's words: shard s's lowest unpicked global
// id (~0: none left) at all[low_at[s]], the sum of global chunk g at all[sum_at[g]].  j >= C: only the total of w (the
// potential) into *total_out.  *fallbacks counts the picks that found total == 0.
__global__ __launch_bounds__(1024) void kmpp_sharded_pick_kernel(const unsigned long long* __restrict__ all, const uint32_t* __restrict__ low_at,
                                                                 uint32_t n_shards, const uint32_t* __restrict__ sum_at,
                                                                 const KmppChunkAt* __restrict__ order, uint32_t n_chunks,
                                                                 const unsigned long long* __restrict__ z, uint32_t j, uint32_t C,
                                                                 KmppPick* __restrict__ pick, uint32_t* __restrict__ fallbacks,
                                                                 unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long sc[1024];
    uint32_t lo, hi;
    unsigned long long excl, incl;
    const unsigned long long total = kmpp_sharded_scan([&](uint32_t k) { return all[sum_at[k]]; }, n_chunks, sc, lo, hi, excl, incl);
    if (j >= C) {
        if (threadIdx.x == 0) {
            *total_out = total;
            KmppPick pk = {0u, 0u, KMPP_PICK_TOTAL << KMPP_PICK_MODE_SHIFT};
            *pick = pk;
        }
        return;
    }
    if (total == 0ull) {   // nothing has weight: the shard that holds the lowest global id not picked before
        if (threadIdx.x == 0) {
            uint32_t owner = 0u;
            unsigned long long best = ~0ull;
            for (uint32_t s = 0; s < n_shards; ++s) {
                const unsigned long long v = all[low_at[s]];
                if (v < best) { best = v; owner = s; }
            }
            KmppPick pk = {owner, 0u, KMPP_PICK_FALLBACK << KMPP_PICK_MODE_SHIFT};
            *pick = pk;
            *fallbacks += 1u;
        }
        return;
    }
    const unsigned long long T = __umul64hi(z[j], total);   // floor(z * total / 2^64) < total
    if (excl <= T && T < incl) {   // exactly one thread
        unsigned long long run = excl;
        for (uint32_t k = lo; k < hi; ++k) {
            const unsigned long long v = all[sum_at[k]];
            if (run + v > T) {
                KmppPick pk = {order[k].shard, order[k].chunk, (T - run) | (KMPP_PICK_WEIGHTED << KMPP_PICK_MODE_SHIFT)};
                *pick = pk;
                break;
            }
            run += v;
        }
    }
}

// Every shard, every seed (one workgroup of 256).  The owner of the pick finds the position — inside its chunk the smallest
// one whose inclusive prefix sum of w exceeds the remainder, or for a fallback the position under its cursor — marks it
// picked, zeroes its weight and writes {global id, 1} and the row into its slot; every other shard writes {-, 0}.  Then the
// cursor moves over picked positions (at most C steps over a call) and *low = the lowest global id not picked, ~0 if none.
__global__ __launch_bounds__(256) void kmpp_sharded_locate_kernel(const float* __restrict__ table, const uint32_t* __restrict__ list,
                                                                  uint32_t n_list, const KmppChunk* __restrict__ desc, uint32_t n_desc,
                                                                  const KmppPick* __restrict__ pick, uint32_t me, IdMap map, uint32_t dim,
                                                                  uint32_t* __restrict__ w, uint32_t* __restrict__ flags,
                                                                  uint32_t* __restrict__ cursor, unsigned long long* __restrict__ low,
                                                                  unsigned long long* __restrict__ slot) {
    __shared__ unsigned long long sc[256];
    __shared__ uint32_t s_p;
    const uint32_t t = threadIdx.x;
    const KmppPick pk = *pick;
    const unsigned long long mode = pk.rem_mode >> KMPP_PICK_MODE_SHIFT;
    const unsigned long long rem = pk.rem_mode & ((1ull << KMPP_PICK_MODE_SHIFT) - 1ull);
    const uint32_t cur0 = *cursor;
    const bool mine = mode != KMPP_PICK_TOTAL && pk.shard == me;   // (the same for every thread)
    if (t == 0) s_p = KMPP_NO_POS;
    __syncthreads();
    if (mine && mode == KMPP_PICK_FALLBACK) {
        if (t == 0) s_p = cur0;
    } else if (mine && pk.chunk < n_desc) {
        const uint32_t first = desc[pk.chunk].first, count = desc[pk.chunk].count;
        const unsigned long long own = t < count ? (unsigned long long)w[first + t] : 0ull;
        sc[t] = own;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            const unsigned long long v = t >= off ? sc[t - off] : 0ull;
            __syncthreads();
            sc[t] += v;
            __syncthreads();
        }
        const unsigned long long incl = sc[t], excl = incl - own;
        if (excl <= rem && rem < incl) s_p = first + t;   // own > 0: exactly one thread
    }
    __syncthreads();
    const uint32_t p = s_p < n_list ? s_p : KMPP_NO_POS;
    if (t == 0) {
        slot[0] = p != KMPP_NO_POS ? id_of_local(map, list[p]) : ~0ull;
        slot[1] = p != KMPP_NO_POS ? 1ull : 0ull;
    }
    if (p != KMPP_NO_POS) {
        const float* src = table + (uint64_t)list[p] * dim;
        float* dst = reinterpret_cast<float*>(slot + 2);
        for (uint32_t e = t; e < dim; e += 256) dst[e] = src[e];
    }
    if (t == 0) {
        if (p != KMPP_NO_POS) {
            flags[p] |= KMPP_PICKED;
            w[p] = 0u;
        }
        uint32_t cur = cur0;
        while (cur < n_list && (cur == p || (flags[cur] & KMPP_PICKED))) ++cur;
        *cursor = cur;
        *low = cur < n_list ? id_of_local(map, list[cur]) : ~0ull;
    }
}

// On the first shard's device (one workgroup of 256): the one slot of the n_shards whose owner flag is set -> rows[j], the
// row into cent[j] (cent may be null) and into the centre the next pass reads.  No flag set: rows[j] = ~0, which the host
// reports.
__global__ __launch_bounds__(256) void kmpp_sharded_select_kernel(const unsigned long long* __restrict__ slots, uint32_t slot_words,
                                                                  uint32_t n_shards, uint32_t dim, uint32_t j,
                                                                  unsigned long long* __restrict__ rows, float* __restrict__ cent,
                                                                  float* __restrict__ centre) {
    __shared__ uint32_t s_owner;
    const uint32_t t = threadIdx.x;
    if (t == 0) s_owner = KMPP_NO_POS;
    __syncthreads();
    for (uint32_t s = t; s < n_shards; s += 256)
        if (slots[(uint64_t)s * slot_words + 1] == 1ull) s_owner = s;
    __syncthreads();
    const uint32_t owner = s_owner;
    if (owner == KMPP_NO_POS) {
        if (t == 0) rows[j] = ~0ull;
        return;
    }
    const unsigned long long* slot = slots + (uint64_t)owner * slot_words;
    const float* src = reinterpret_cast<const float*>(slot + 2);
    if (t == 0) rows[j] = slot[0];
    for (uint32_t e = t; e < dim; e += 256) {
        const float v = src[e];
        if (cent) cent[(uint64_t)j * dim + e] = v;
        centre[e] = v;
    }
}

}  // namespace mi
