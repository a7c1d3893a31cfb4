// kmeans_seed_kernels.h — device code of mi_knn_kmeans_seed: k-means++ seeding over S candidate rows, exact.
//
// Per candidate position p the device keeps D[p] (the smallest distance to a centre chosen so far, NaN = unset), the
// integer weight w[p] = floor(clamp(D[p], 0, 2) * 2^30) and two flag bits (usable, picked).  A pass is one fp32 sweep over
// the candidate rows against the last centre: it lowers D, rewrites w and leaves one uint64 sum of w per chunk of
// consecutive positions.  A pick turns a random 64-bit z into the threshold T = floor(z * total / 2^64) and finds the
// smallest p whose inclusive prefix sum of w exceeds T: first among the chunk sums, then inside the chunk.  Everything the
// choice depends on is an integer (sums of uint32 in uint64: any order gives the same value) or a distance with the search's
// bits (the written-out pair-distance block of assign_rescore_kernel: the centre is the query, the candidate the streamed
// row), so the picks can be restated on the host to the bit.  No float atomics, no atomics at all.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "knn_shared.h"

namespace mi {

constexpr uint32_t KMPP_USABLE = 1u, KMPP_PICKED = 2u;
constexpr uint32_t KMPP_CHUNK = 256;         // positions of a chunk: a multiple of this (16 per 16-lane group and step)
constexpr uint32_t KMPP_MAX_CHUNKS = 8192;   // what the one workgroup of a pick scans before it enters a chunk

// Workgroup b owns the positions [b * chunk, (b + 1) * chunk) (chunk a multiple of 16), a 16-lane group one position per
// step.  FIRST: the pass before pick 0 — the row against itself decides "usable" (a non-NaN self-distance), D = unset,
// w = usable.  Otherwise the centre is the candidate at position *centre, where the previous pick wrote it.
template <int NCH, bool FIRST = false>
__global__ __launch_bounds__(256) void kmpp_pass_kernel(const float* __restrict__ table, const uint32_t* __restrict__ list, uint32_t S,
                                                        uint32_t chunk, const uint32_t* __restrict__ centre, float* __restrict__ D,
                                                        uint32_t* __restrict__ w, uint32_t* __restrict__ flags,
                                                        unsigned long long* __restrict__ chunk_sum) {
    constexpr int DIM = NCH * 64;
    __shared__ unsigned long long part[16];
    const int lane = threadIdx.x & 63, i = lane & 15, g = threadIdx.x >> 4;
    const uint64_t p0 = (uint64_t)blockIdx.x * chunk;
    f32x4 qf[NCH];
    float sq = 0.0f;  // sqrt(q.q), same summation order as a row
    if (!FIRST) {
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)list[*centre] * DIM) + i;
#pragma unroll
        for (int t = 0; t < NCH; ++t) qf[t] = pa[16 * t];
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
        sq = sqrtf(a.sumsq());
    }
    unsigned long long sum = 0ull;
    // (whole waves stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t o = (uint32_t)g; o < chunk; o += 16) {
        const uint64_t p1 = p0 + o;
        const bool live = p1 < S;
        const uint32_t p = live ? (uint32_t)p1 : S - 1;
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

// One workgroup of 1024 threads over n values val(0 .. n - 1): thread t sums a contiguous piece, the pieces are scanned in
// LDS.  Returns the total; lo / hi = the thread's piece, excl = the sum of everything before it, incl = excl + its own.
template <class F>
__device__ __forceinline__ unsigned long long kmpp_scan(F val, uint32_t n, unsigned long long* sc, uint32_t& lo, uint32_t& hi,
                                                        unsigned long long& excl, unsigned long long& incl) {
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint64_t l = (uint64_t)t * per, h = l + per;
    lo = (uint32_t)(l < n ? l : n);
    hi = (uint32_t)(h < n ? h : n);
    unsigned long long own = 0ull;
    for (uint32_t k = lo; k < hi; ++k) own += val(k);
    __syncthreads();   // (sc may still be read from a previous scan)
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

// Pick j (one workgroup of 1024).  j == C: only the total of w (the potential) into *total_out.
// state = {cursor: every position below it is picked, fallback picks so far}.
__global__ __launch_bounds__(1024) void kmpp_pick_kernel(const unsigned long long* __restrict__ chunk_sum, uint32_t n_chunks, uint32_t chunk,
                                                         uint32_t S, uint32_t* __restrict__ w, uint32_t* __restrict__ flags,
                                                         const unsigned long long* __restrict__ z, uint32_t j, uint32_t C,
                                                         uint32_t* __restrict__ picks, uint32_t* __restrict__ state,
                                                         unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long sc[1024];
    __shared__ unsigned long long s_left;
    __shared__ uint32_t s_chunk;
    uint32_t lo, hi;
    unsigned long long excl, incl;
    const unsigned long long total = kmpp_scan([&](uint32_t k) { return chunk_sum[k]; }, n_chunks, sc, lo, hi, excl, incl);
    if (j >= C) {
        if (threadIdx.x == 0) *total_out = total;
        return;
    }
    if (total == 0ull) {   // nothing has weight: the lowest position not picked before
        if (threadIdx.x == 0) {
            uint32_t p = state[0];
            while (p < S - 1 && (flags[p] & KMPP_PICKED)) ++p;
            picks[j] = p;
            flags[p] |= KMPP_PICKED;
            w[p] = 0u;
            state[0] = p + 1;
            state[1] += 1u;
        }
        return;
    }
    const unsigned long long T = __umul64hi(z[j], total);   // floor(z * total / 2^64) < total
    if (threadIdx.x == 0) { s_chunk = 0u; s_left = 0ull; }
    __syncthreads();
    if (excl <= T && T < incl) {   // exactly one thread
        unsigned long long run = excl;
        for (uint32_t k = lo; k < hi; ++k) {
            const unsigned long long v = chunk_sum[k];
            if (run + v > T) { s_chunk = k; s_left = T - run; break; }
            run += v;
        }
    }
    __syncthreads();
    const uint32_t first = s_chunk * chunk;   // (s_chunk < n_chunks: first < S)
    const unsigned long long Tc = s_left;
    const uint32_t n = S - first < chunk ? S - first : chunk;
    kmpp_scan([&](uint32_t k) { return (unsigned long long)w[first + k]; }, n, sc, lo, hi, excl, incl);
    if (excl <= Tc && Tc < incl) {
        unsigned long long run = excl;
        for (uint32_t k = lo; k < hi; ++k) {
            const unsigned long long v = w[first + k];
            if (run + v > Tc) {
                const uint32_t p = first + k;
                picks[j] = p;
                flags[p] |= KMPP_PICKED;
                w[p] = 0u;
                break;
            }
            run += v;
        }
    }
}

// the picked rows' fp32 values, in pick order: workgroup j copies one row
__global__ __launch_bounds__(256) void kmpp_gather_kernel(const float* __restrict__ table, const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ picks, uint32_t dim, float* __restrict__ out) {
    const float* src = table + (uint64_t)list[picks[blockIdx.x]] * dim;
    for (uint32_t e = threadIdx.x; e < dim; e += 256) out[(uint64_t)blockIdx.x * dim + e] = src[e];
}

}  // namespace mi
