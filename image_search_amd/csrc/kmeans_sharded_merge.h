// kmeans_sharded_merge.h — the exchange between the shards that mi_knn_sharded_kmeans (kmeans_sharded.hip) and
// mi_knn_sharded_summarize (summary_sharded.hip) share: the integer sums and sizes of shards 1 .. S - 1 are copied to shard
// 0's device and added into shard 0's, the centroids are formed there and copied back to every shard.  One function, so that
// both calls enqueue the same launches and copies in the same order.  The rules without HIP in them: kmeans_fixed_host.h.
#pragma once
#include <algorithm>
#include <mutex>
#include <vector>

#include "assign_kernels.h"
#include "common.h"
#include "handles.h"
#include "kmeans_update.h"
#include "sharded_call.h"
#include "two_stage.h"

namespace mi {

constexpr uint64_t KM_MERGE_CHUNK = 1ull << 21;   // 64-bit sums copied to shard 0's device at a time (16 MB)

// what one shard brings to the exchange; the device memory belongs to the call
struct KmPart {
    mi_knn* sh = nullptr;
    hipStream_t s = nullptr;
    Event ev;                       // shard >= 1: its sums are in place; shard 0: the centroids are
    float* d_vec = nullptr;         // [C][dim]: the centroids
    long long* d_S = nullptr;       // [C][dim] / [C]: the shard's sums and sizes (zeros where it has no rows)
    uint32_t* d_n = nullptr;
};

// where shard 0 stages another shard's sums and sizes; shard 0's device selected
inline void km_merge_staging(Scratch& scratch, uint32_t C, uint32_t dim, long long** d_in, uint32_t** d_nin) {
    *d_in = (long long*)scratch.get((size_t)std::min<uint64_t>((uint64_t)C * dim, KM_MERGE_CHUNK) * sizeof(long long));
    *d_nin = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
}

// Every part's d_S / d_n (behind the event the shards >= 1 recorded on their streams) -> the merged sums and sizes in part
// 0's, the centroids in every part's d_vec.  Enqueues only; *merges += the merge launches.
inline void km_merge_and_broadcast(const std::vector<KmPart*>& st, uint32_t C, uint32_t dim, long long* d_in, uint32_t* d_nin,
                                   uint64_t* merges) {
    const uint32_t S = (uint32_t)st.size();
    const uint64_t el = (uint64_t)C * dim;
    KmPart& z = *st[0];
    {
        std::lock_guard<std::mutex> l(z.sh->mu);
        DeviceGuard g(z.sh->device);
        const uint32_t max_blocks = (uint32_t)std::max(z.sh->n_cu, 1) * 8u;
        for (uint32_t si = 1; si < S; ++si) {
            KmPart& x = *st[si];
            HIP_CHECK(hipStreamWaitEvent(z.s, x.ev, 0));
            copy_between(d_nin, z.sh->device, x.d_n, x.sh->device, (size_t)C * sizeof(uint32_t), z.s);
            for (uint64_t e0 = 0; e0 < el; e0 += KM_MERGE_CHUNK) {
                const uint64_t n = std::min<uint64_t>(KM_MERGE_CHUNK, el - e0);
                copy_between(d_in, z.sh->device, x.d_S + e0, x.sh->device, (size_t)n * sizeof(long long), z.s);
                const uint32_t blocks = (uint32_t)std::min<uint64_t>(max_blocks, (n + 255) / 256);
                hipLaunchKernelGGL(km_merge_fixed_kernel, dim3(blocks), dim3(256), 0, z.s, z.d_S + e0, (const long long*)d_in, n, z.d_n,
                                   (const uint32_t*)d_nin, e0 == 0 ? C : 0u);   // (the sizes ride with the first chunk)
                HIP_CHECK(hipGetLastError());
                ++*merges;
            }
        }
        KmUpdate::centroids_fixed(z.s, z.d_S, z.d_n, C, dim, z.d_vec);
        HIP_CHECK(hipEventRecord(z.ev, z.s));
    }
    for (uint32_t si = 1; si < S; ++si) {
        KmPart& x = *st[si];
        std::lock_guard<std::mutex> l(x.sh->mu);
        DeviceGuard g(x.sh->device);
        HIP_CHECK(hipStreamWaitEvent(x.s, z.ev, 0));
        copy_between(x.d_vec, x.sh->device, z.d_vec, z.sh->device, (size_t)el * sizeof(float), x.s);
    }
}

}  // namespace mi
