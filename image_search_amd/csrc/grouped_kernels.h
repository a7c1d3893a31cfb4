// grouped_kernels.h — device code of mi_knn_search_grouped: the best row per group and the number of in-window rows per group,
// from the 32-bit distance keys knn_page_scan_kernel<NCH, 1> leaves (one per row or list entry, 0xFFFFFFFF outside the window).
//
// The reduction is NOT fused into the scan.  The scan reads 3 072 B per row (dim 768) and is bound by HBM; these passes touch
// 12 B per row (key, row, group).  Fused, up to one same-address atomic per row would sit inside the HBM-bound loop — with one
// heavy group that is 10^7 atomics on one word, which a single L2 channel retires at some tens per microsecond.  Here the heavy
// group costs one LDS atomic per row and one global atomic per workgroup.
//
// Every value is an integer and every update is a min or an add, so the slots hold the same bits in any arrival order:
//   best[g] = min over the in-window rows of group g of (key32 << 32 | local row) — the search's own 64-bit key
//   cnt[g]  = the number of those rows
// Rows without a group (MI_KNN_NO_GROUP) take no slot: each is its own representative.
// All three passes walk the keys in strides of 256 per workgroup; e is wave-uniform apart from the lane, so ballots are safe.
#pragma once
#include "../../include/mi355clip.h"
#include "knn_shared.h"

namespace mi {

constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;
constexpr uint32_t GROUP_KEY_OUT = 0xFFFFFFFFu;   // the scan's "not in the window"

// one lane's entry: the row of position e and its group, or GROUP_NONE when the entry takes no slot
struct GroupEntry {
    uint32_t key, row, group;
};
__device__ __forceinline__ GroupEntry group_entry(const uint32_t* __restrict__ keys32, uint64_t n, const uint32_t* __restrict__ list,
                                                  const uint32_t* __restrict__ groups, uint32_t n_groups, uint64_t e) {
    GroupEntry x{GROUP_KEY_OUT, 0u, GROUP_NONE};
    if (e >= n) return x;
    x.key = keys32[e];
    if (x.key == GROUP_KEY_OUT) return x;
    x.row = list ? list[e] : (uint32_t)e;
    const uint32_t g = groups ? groups[x.row] : GROUP_NONE;
    x.group = g < n_groups ? g : GROUP_NONE;   // (a group id is always < n_groups; anything else is treated as "none" throughout)
    return x;
}

// grid: any number of 256-thread workgroups.  best [n_groups] preset to all ones, cnt [n_groups] to zero.
// LDS == 1: n_groups * 12 bytes of dynamic LDS (n_groups <= GROUP_LDS_MAX): block-private tables built with LDS atomics
//           (ds_min_u64, ds_add_u32), then every touched slot goes out with one global atomicMin and one atomicAdd.
// LDS == 0: straight to the global slots.  The atomicMin is issued only when the lane's key is below the value it has just
//           read (the slot only ever decreases, so a stale read can cost a needless atomic, never a missed one); the adds of
//           equal groups inside a wave are combined: a wave-uniform loop over the distinct groups of the 64 lanes, one add of
//           the popcount each.
template <int LDS>
__global__ __launch_bounds__(256, 2) void group_reduce_kernel(const uint32_t* __restrict__ keys32, uint64_t n,
                                                              const uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ groups, uint32_t n_groups,
                                                              unsigned long long* __restrict__ best, uint32_t* __restrict__ cnt) {
    extern __shared__ unsigned long long group_lds[];
    unsigned long long* l_best = group_lds;
    uint32_t* l_cnt = reinterpret_cast<uint32_t*>(group_lds + n_groups);
    if constexpr (LDS == 1) {
        for (uint32_t g = threadIdx.x; g < n_groups; g += 256) {
            l_best[g] = ~0ull;
            l_cnt[g] = 0u;
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {
        const GroupEntry x = group_entry(keys32, n, list, groups, n_groups, base + threadIdx.x);
        const bool act = x.group != GROUP_NONE;
        const unsigned long long key = ((unsigned long long)x.key << 32) | x.row;
        if constexpr (LDS == 1) {
            if (act) {
                atomicMin(&l_best[x.group], key);
                atomicAdd(&l_cnt[x.group], 1u);
            }
        } else {
            if (act && key < __hip_atomic_load(&best[x.group], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&best[x.group], key);
            unsigned long long todo = __ballot(act);
            while (todo) {   // wave-uniform
                const int leader = __ffsll((long long)todo) - 1;
                const uint32_t lg = (uint32_t)__shfl((int)x.group, leader, 64);
                const unsigned long long same = __ballot(act && x.group == lg);
                if (lane == leader) atomicAdd(&cnt[lg], (uint32_t)__popcll(same));
                todo &= ~same;
            }
        }
    }
    if constexpr (LDS == 1) {
        __syncthreads();
        for (uint32_t g = threadIdx.x; g < n_groups; g += 256) {
            const uint32_t c = l_cnt[g];
            if (c) {
                atomicMin(&best[g], l_best[g]);
                atomicAdd(&cnt[g], c);
            }
        }
    }
}

// A row that holds a group and is not that group's best leaves the selection: its key32 becomes 0xFFFFFFFF.  What stays in
// the window are the representatives — the best row of every matched group and every in-window row without a group — counted
// with ballots, one atomic add per wave.  groups == nullptr or n_groups == 0: nothing is rewritten, everything in the window
// is counted.
__global__ __launch_bounds__(256) void group_mark_kernel(uint32_t* __restrict__ keys32, uint64_t n, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ groups, uint32_t n_groups,
                                                         const unsigned long long* __restrict__ best,
                                                         unsigned long long* __restrict__ n_reps) {
    uint32_t reps = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {
        const uint64_t e = base + threadIdx.x;
        const GroupEntry x = group_entry(keys32, n, list, groups, n_groups, e);
        bool rep = x.key != GROUP_KEY_OUT;
        if (rep && x.group != GROUP_NONE && ((((unsigned long long)x.key) << 32) | x.row) != best[x.group]) {
            keys32[e] = GROUP_KEY_OUT;
            rep = false;
        }
        reps += (uint32_t)__popcll(__ballot(rep));
    }
    if ((threadIdx.x & 63) == 0 && reps) atomicAdd(n_reps, (unsigned long long)reps);
}

// The k sorted keys (distance key << 32 | local row, ascending) -> idx / dist / group / members; one thread per result slot.
// A key whose distance word is 0xFFFFFFFF is padding.  members: cnt of the hit's group, 1 for a row without one.
__global__ void group_finish_kernel(const uint64_t* __restrict__ keys, uint32_t k, IdMap map, const uint32_t* __restrict__ groups,
                                    uint32_t n_groups, const uint32_t* __restrict__ cnt, uint64_t* __restrict__ idx,
                                    uint64_t* __restrict__ members, float* __restrict__ dist, uint32_t* __restrict__ group) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint64_t key = keys[j];
    const bool hit = (uint32_t)(key >> 32) != 0xFFFFFFFFu;
    uint32_t g = GROUP_NONE;
    if (hit && groups && n_groups) {
        g = groups[(uint32_t)key];
        if (g >= n_groups) g = GROUP_NONE;
    }
    idx[j] = hit ? id_of_local(map, (uint32_t)key) : MI_KNN_NO_ID;
    dist[j] = hit ? u32_to_dist((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
    group[j] = g;
    members[j] = !hit ? 0ull : g == GROUP_NONE ? 1ull : (uint64_t)cnt[g];
}

// members of the sharded call's winners: out[j] += this shard's cnt of group[j] (nothing for GROUP_NONE or a group this shard
// has never seen)
__global__ void group_gather_kernel(const uint32_t* __restrict__ group, uint32_t k, const uint32_t* __restrict__ cnt, uint32_t n_groups,
                                    uint32_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint32_t g = group[j];
    out[j] = g < n_groups ? cnt[g] : 0u;
}

}  // namespace mi
