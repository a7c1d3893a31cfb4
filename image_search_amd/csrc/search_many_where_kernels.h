// search_many_where_kernels.h — device code of the narrowed many-query calls (mi_knn_search_many_where,
// mi_knn_neighbors_where, mi_knn_propose_groups): the mask builder in front of stage 1 and the vote behind stage 2.  Stage 1,
// the superset bound and the rescore are search_many_kernels.h's, as they stand.
//
// many_mask_kernel turns a predicate (where_pred.h's row test) and a rule on the group column into a bitmap of the rows
// that must NOT take part, in the deletion bitmap's format: search_many_tiles_kernel takes it in place of `tomb` (columns) or
// of `q_tomb` (query rows) and gives a marked row weight 0 — it never emits and never enters a slot.  The slots are therefore
// filled from unmasked columns only, which is what a table holding only those rows would do: the superset argument of
// search_many_kernels.h stands with "live" read as "unmasked".
//
// many_vote_kernel reads a strip's stage-2 slots (a row's k nearest voters, ascending) and tallies their groups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "knn_shared.h"
#include "where_pred.h"

namespace mi {

constexpr uint32_t VOTE_MAX_K = 16;
constexpr uint32_t VOTE_NO_GROUP = 0xFFFFFFFFu;   // MI_KNN_NO_GROUP

// the rule on the group column beside the predicate: none / the row has a group and it is not x / the row's group is x
// (x = no group: the rows without one).  A table without a group column: every row has no group.
enum MaskGroupRule : uint32_t { MASK_GROUP_ANY = 0, MASK_GROUP_OTHER = 1, MASK_GROUP_IS = 2 };

// mask [(rows + 63) / 64] words, bit r set = row r stays out: deleted, failing the predicate or failing the group rule; the
// bits at and beyond `rows` in the last word are set.  *clear += the clear bits (the rows that take part).  One lane per
// row, one wave per word; grid = ceil(words / 4) workgroups of 256.
__global__ __launch_bounds__(256) void many_mask_kernel(WherePred p, const unsigned long long* __restrict__ tags,
                                                        const long long* __restrict__ stamps, const uint32_t* __restrict__ groups,
                                                        const unsigned long long* __restrict__ tomb, uint64_t rows, uint32_t rule,
                                                        uint32_t x, uint64_t* __restrict__ mask, unsigned long long* __restrict__ clear) {
    const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool out = !where_match(p, tags, stamps, groups, tomb, row, rows);   // (false beyond `rows`: out)
    if (!out && rule != MASK_GROUP_ANY) {
        const uint32_t g = groups ? groups[row] : VOTE_NO_GROUP;
        out = rule == MASK_GROUP_OTHER ? (g == VOTE_NO_GROUP || g == x) : g != x;
    }
    const unsigned long long word = __ballot(out);
    if ((threadIdx.x & 63) == 0 && (row >> 6) < (rows + 63) / 64) {
        mask[row >> 6] = word;
        const uint32_t n = (uint32_t)__popcll(~word);
        if (n) atomicAdd(clear, (unsigned long long)n);
    }
}

// A strip's slots ([n_local][m] keys, ascending, KEY_MAX = none; key = distance key << 32 | local table row of a voter) ->
// the proposal of strip row r = the table's local row q_local0 + r, written at that row of group / votes / heard / dist
// (votes / heard / dist nullable).  L = the row's entries up to the first key beyond the window (distance key <= hi_key,
// inclusive); the winner = the group with the most entries in L, among equal counts the one whose first entry stands
// earliest.  A row whose bit is set in q_mask (not an asker) and a row with an empty L get no proposal.
// totals[0] += rows with a proposal, totals[1] += those with votes == heard.  One lane per strip row.
__global__ __launch_bounds__(256) void many_vote_kernel(const unsigned long long* __restrict__ slot, const uint64_t* __restrict__ q_mask,
                                                        uint32_t q_local0, uint32_t n_local, uint32_t m, uint32_t hi_key,
                                                        const uint32_t* __restrict__ groups, uint32_t* __restrict__ group,
                                                        uint32_t* __restrict__ votes, uint32_t* __restrict__ heard,
                                                        float* __restrict__ dist, unsigned long long* __restrict__ totals) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    uint32_t proposed = 0, unanimous = 0;
    if (r < n_local) {
        const uint32_t self = q_local0 + r;
        const bool asks = !((q_mask[self >> 6] >> (self & 63)) & 1ull);
        uint32_t g[VOTE_MAX_K], key_of[VOTE_MAX_K], n = 0;
        if (asks) {
            const unsigned long long* p = slot + (size_t)r * m;
#pragma unroll
            for (uint32_t j = 0; j < VOTE_MAX_K; ++j) {
                g[j] = VOTE_NO_GROUP; key_of[j] = 0xFFFFFFFFu;
                if (j < m && n == j) {   // (n == j: nothing before it ended the list)
                    const unsigned long long key = p[j];
                    if (key != KEY_MAX && (uint32_t)(key >> 32) <= hi_key) {
                        g[j] = groups[(uint32_t)key];
                        key_of[j] = (uint32_t)(key >> 32);
                        n = j + 1;
                    }
                }
            }
        }
        // the tally: entry i stands for its group when no earlier entry holds the same; ascending i and a strict compare give
        // the earliest among equal counts
        uint32_t win = VOTE_NO_GROUP, win_n = 0, win_key = 0;
        if (asks) {
#pragma unroll
            for (uint32_t i = 0; i < VOTE_MAX_K; ++i) {
                if (i < n) {
                    uint32_t cnt = 0;
                    bool first = true;
#pragma unroll
                    for (uint32_t j = 0; j < VOTE_MAX_K; ++j) {
                        const bool same = j < n && g[j] == g[i];
                        cnt += same ? 1u : 0u;
                        first = first && !(same && j < i);
                    }
                    if (first && cnt > win_n) { win = g[i]; win_n = cnt; win_key = key_of[i]; }
                }
            }
        }
        group[self] = win;
        if (votes) votes[self] = win_n;
        if (heard) heard[self] = n;
        if (dist) dist[self] = win_n ? u32_to_dist(win_key) : __uint_as_float(0x7F800000u);
        proposed = win_n ? 1u : 0u;
        unanimous = (win_n && win_n == n) ? 1u : 0u;
    }
    // one atomic per wave and counter
    uint32_t packed = proposed | (unanimous << 16);   // (at most 64 of each per wave)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) packed += __shfl_xor(packed, d, 64);
    if ((threadIdx.x & 63) == 0) {
        if (packed & 0xFFFFu) atomicAdd(totals, (unsigned long long)(packed & 0xFFFFu));
        if (packed >> 16) atomicAdd(totals + 1, (unsigned long long)(packed >> 16));
    }
}

}  // namespace mi
