// representatives_kernels.h — device code of mi_knn_representatives: farthest-first traversal (the greedy k-center picks) of
// every group of rows at once.
//
// Per member row r the device keeps K[r], the smallest distance KEY to a pick of its group so far (0xFFFFFFFF = none yet, or
// only NaN), rep[r], the pick that set it, and a picked flag.  Per group it keeps the latest pick (the centre of the next
// round), the number of picks, a done flag and one 64-bit slot.  The members are bucketed by group with the k-means update's
// walk (kmeans_update.h: d_sorted / d_start / d_seg, segments of KM_SEG members, a segment inside one group), as
// summary_dist_kernel consumes them.
//
// Round j = 1 .. m is two launches:
//   rep_round_kernel    one workgroup per segment: the group's centre (pick j - 1) in registers, each member row read once,
//                       d(centre, member) in the search's bits (the written-out pair-distance block of kmpp_pass_kernel: the
//                       pick is the query, the member the streamed row), K lowered by a strict compare on keys, and the
//                       candidates (not picked, K a number) folded to one word rep_word(K, row) — lanes, waves through LDS,
//                       then ONE 64-bit atomicMax on the group's slot.  A done group's workgroups leave without reading a row.
//   rep_advance_kernel  one lane per group: reads and clears the slot; round m only closes the group (its K now holds every
//                       pick); otherwise the word's row becomes pick j if its key passes the min_gap window, else the group is
//                       done.  The round's picks are counted in one word.
// After the last round rep_reach_kernel walks the segments once more without touching the table: rep_dist from K, and the
// largest number key of every group by the same fold.
//
// Every decision is an integer compare on search keys or a 64-bit integer max whose result does not depend on the order of
// arrival: no float atomics, no per-row atomics, the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assign_kernels.h"
#include "knn_shared.h"
#include "representatives_host.h"

namespace mi {

// words of the call: [0] start entries that are no member of their (non-empty) group, [1] the lowest such group
constexpr int RW_BAD = 0, RW_BAD_GROUP = 1, RW_WORDS = 2;

// the group of segment g: the last c with seg[c] <= g
__device__ __forceinline__ uint32_t rep_group_of(const uint32_t* __restrict__ seg, uint32_t C, uint32_t g) {
    uint32_t lo = 0, hi = C;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// a workgroup's 256 values -> their max in thread 0 (lanes by shuffles, the four waves through LDS)
__device__ __forceinline__ unsigned long long rep_fold_max(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = umax64(v, shfl_xor64(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) v = umax64(v, red[w]);
    }
    return v;
}

// Pick 0, one lane per group: start_rows[c] (start given: it must be a member of c — a row of the table with label c whose
// flag is not NaN, summary_prepare_kernel's "live and usable"), else the group's first member (the lowest row = the lowest id).
// An empty group is done at once and its start entry is not looked at.  made[0] += groups that picked.
__global__ __launch_bounds__(256) void rep_start_kernel(const uint32_t* __restrict__ labels, const float* __restrict__ flag,
                                                        const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ start,
                                                        const uint32_t* __restrict__ start_rows, uint32_t n_rows, uint32_t C, uint32_t m,
                                                        uint32_t* __restrict__ centre, uint32_t* __restrict__ done,
                                                        uint32_t* __restrict__ n_picked, uint32_t* __restrict__ picks,
                                                        uint32_t* __restrict__ picked, uint32_t* __restrict__ made,
                                                        uint32_t* __restrict__ words) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    centre[c] = REP_NO_ROW;
    n_picked[c] = 0u;
    done[c] = 1u;
    if (start[c + 1] == start[c]) return;
    uint32_t r = sorted[start[c]];
    if (start_rows) {
        r = start_rows[c];
        bool ok = r < n_rows;
        if (ok) {
            const float f = flag[r];
            ok = labels[r] == c && f == f;
        }
        if (!ok) {
            atomicAdd(words + RW_BAD, 1u);
            atomicMin(words + RW_BAD_GROUP, c);
            return;
        }
    }
    picks[(size_t)c * m] = r;
    picked[r] = 1u;
    centre[c] = r;
    n_picked[c] = 1u;
    done[c] = 0u;
    atomicAdd(made, 1u);
}

// Round j (index = j - 1: the pick being measured), workgroup g = segment g of the walk.
template <int NCH>
__global__ __launch_bounds__(256) void rep_round_kernel(const float* __restrict__ table, const uint32_t* __restrict__ sorted,
                                                        const uint32_t* __restrict__ start, const uint32_t* __restrict__ seg, uint32_t C,
                                                        uint32_t index, const uint32_t* __restrict__ centre,
                                                        const uint32_t* __restrict__ done, const uint32_t* __restrict__ picked,
                                                        uint32_t* __restrict__ K, uint32_t* __restrict__ rep,
                                                        unsigned long long* __restrict__ slots, unsigned long long* __restrict__ rows_read) {
    constexpr int DIM = NCH * 64;
    __shared__ unsigned long long red[4];
    const uint32_t g = blockIdx.x;
    if (g >= seg[C]) return;
    const uint32_t c = rep_group_of(seg, C, g);
    if (done[c]) return;   // (the whole workgroup: nothing below is reached by a part of it)
    const uint32_t first = start[c] + (g - seg[c]) * KM_SEG;
    const uint32_t n = min((uint32_t)KM_SEG, start[c + 1] - first);
    const int lane = threadIdx.x & 63, i = lane & 15, grp = threadIdx.x >> 4;
    // lane i of a 16-lane group holds elements 64 t + 4 i .. + 3 of the centre: the query
    f32x4 qf[NCH];
    {
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)centre[c] * DIM) + i;
#pragma unroll
        for (int t = 0; t < NCH; ++t) qf[t] = pa[16 * t];
    }
    float sq;   // sqrt(q.q), same summation order as a row
    {
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
        sq = sqrtf(a.sumsq());
    }
    unsigned long long best = REP_SLOT_EMPTY;
    // (whole 16-lane groups stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t m0 = 0; m0 < n; m0 += 16) {
        const uint32_t mm = m0 + (uint32_t)grp;
        const bool live = mm < n;
        const uint32_t r = sorted[first + (live ? mm : 0u)];
        const f32x4* pb = reinterpret_cast<const f32x4*>(table + (uint64_t)r * DIM) + i;
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], pb[16 * t]);
        const float d = a.dot(), s = a.sumsq();
        const float dist = 1.0f - d / (sq * sqrtf(s));
        if (live && i == 0) {
            const uint32_t key = dist_to_u32(dist);
            uint32_t k = K[r];
            if (key < k) {
                k = key;
                K[r] = k;
                rep[r] = index;
            }
            if (k != 0xFFFFFFFFu && !picked[r]) best = umax64(best, rep_word(k, r));
        }
    }
    best = rep_fold_max(best, red);
    if (threadIdx.x == 0) {
        if (best != REP_SLOT_EMPTY) atomicMax(slots + c, best);
        atomicAdd(rows_read + index + 1, (unsigned long long)n);
    }
}

// Round j, one lane per group: pick j from the slot, or the end of the group.  made[j] += the picks of this round.
__global__ __launch_bounds__(256) void rep_advance_kernel(uint32_t C, uint32_t m, uint32_t j, uint32_t window_key, uint32_t bounded,
                                                          unsigned long long* __restrict__ slots, uint32_t* __restrict__ centre,
                                                          uint32_t* __restrict__ done, uint32_t* __restrict__ n_picked,
                                                          uint32_t* __restrict__ picks, float* __restrict__ gap,
                                                          uint32_t* __restrict__ picked, uint32_t* __restrict__ made) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    bool took = false;
    if (c < C && !done[c]) {
        const unsigned long long word = slots[c];
        slots[c] = REP_SLOT_EMPTY;
        if (j < m && rep_takes(word, window_key, bounded)) {
            const uint32_t r = rep_word_row(word);
            picks[(size_t)c * m + j] = r;
            gap[(size_t)c * m + j] = u32_to_dist(rep_word_key(word));
            picked[r] = 1u;
            centre[c] = r;
            n_picked[c] = j + 1u;
            took = true;
        } else {
            done[c] = 1u;
        }
    }
    const unsigned long long mask = __ballot(took);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(made + j, (uint32_t)__popcll(mask));
}

// After the last round, workgroup g = segment g: rep_dist[r] = the distance of K[r] for every member, and the group's largest
// number key into reach[c] by the rounds' fold.  Reads no row of the table.
__global__ __launch_bounds__(256) void rep_reach_kernel(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ start,
                                                        const uint32_t* __restrict__ seg, uint32_t C, const uint32_t* __restrict__ K,
                                                        float* __restrict__ rep_dist, unsigned long long* __restrict__ reach) {
    __shared__ unsigned long long red[4];
    const uint32_t g = blockIdx.x;
    if (g >= seg[C]) return;
    const uint32_t c = rep_group_of(seg, C, g);
    const uint32_t first = start[c] + (g - seg[c]) * KM_SEG;
    const uint32_t n = min((uint32_t)KM_SEG, start[c + 1] - first);
    unsigned long long best = REP_SLOT_EMPTY;
    for (uint32_t mm = threadIdx.x; mm < n; mm += 256) {
        const uint32_t r = sorted[first + mm];
        const uint32_t k = K[r];
        rep_dist[r] = u32_to_dist(k);
        if (k != 0xFFFFFFFFu) best = umax64(best, rep_word(k, r));
    }
    best = rep_fold_max(best, red);
    if (threadIdx.x == 0 && best != REP_SLOT_EMPTY) atomicMax(reach + c, best);
}

}  // namespace mi
