// summary_sharded_kernels.h — device code of mi_knn_sharded_summarize beside the single table's (summary_kernels.h, which
// every shard runs unchanged): a shard's per-group slots from local rows to global ids, and the slots of another shard folded
// into shard 0's.  One thread owns a group in both, so neither needs an atomic: what orders them against summary_dist_kernel
// and against the copies between the shards is the stream.  The rules and why they hold: summary_sharded_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ids.h"
#include "knn_shared.h"
#include "summary_sharded_host.h"

namespace mi {

// slots [4][C] of one shard, as summary_dist_kernel left them: the rows in planes 0 and 1 become global ids
static __global__ __launch_bounds__(256) void summary_globalize_kernel(unsigned long long* __restrict__ slots, uint32_t C, IdMap map) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    slots[c] = summary_globalize_min(slots[c], map);
    slots[(size_t)C + c] = summary_globalize_max(slots[(size_t)C + c], map);
}

// dst [4][C] (shard 0's) takes in src [4][C] (another shard's, staged on shard 0's device): min, max, sum, sum
static __global__ __launch_bounds__(256) void summary_merge_slots_kernel(unsigned long long* __restrict__ dst,
                                                                         const unsigned long long* __restrict__ src, uint32_t C) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    dst[c] = umin64(dst[c], src[c]);
    dst[(size_t)C + c] = umax64(dst[(size_t)C + c], src[(size_t)C + c]);
    dst[(size_t)2 * C + c] += src[(size_t)2 * C + c];
    dst[(size_t)3 * C + c] += src[(size_t)3 * C + c];
}

}  // namespace mi
