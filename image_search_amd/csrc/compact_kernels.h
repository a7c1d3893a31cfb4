// compact_kernels.h — the device side of mi_knn_compact (compact.hip; the host-only rules: compact_host.h).
//
// Destination row j of the compacted table holds what source row src[j] held: the j-th live row, src[j] = j + (the deleted
// rows below it).  src ascends strictly and src[j] >= j.  Rows below the first deleted row have src[j] == j and are neither
// read nor written; the others move IN PLACE, in ascending chunks [j0, j1) of destination rows, each launch behind the last
// on one stream.
//
// Why no move destroys a row that is still needed.  A chunk writes rows [j0, j1) only.
//   - Chunks in front of it have finished (stream order) and read sources below theirs.
//   - A LATER chunk reads src[j'] for j' >= j1, and src[j'] >= j' >= j1: outside [j0, j1).  So writing [j0, j1) never
//     destroys a later chunk's source, whichever way this chunk is moved.
//   - The chunk ITSELF reads src[j0 .. j1).  If src[j0] >= j1 every one of its sources is >= j1 (they ascend), none lies in
//     [j0, j1), and its lanes may read and write in any order: it is gathered straight into place (one launch).  Otherwise
//     a lane could overwrite a row another lane has yet to read, so the chunk is gathered into the staging buffer and a
//     second launch copies the buffer to [j0, j1) (staged; the buffer holds one chunk).
// The decision is compact_plan's (compact_host.h); tests/cpp/test_compact_host.cpp replays plans with adversarial write orders.
//
// compact_move_kernel is a plain copy: a flat grid-stride index over (destination row, 16-byte piece), one 16-byte load and one
// 16-byte vector store per lane and step, both non-temporal (every byte is touched once, the table is far larger than L2).  A
// row is dim x 4 bytes with dim % 64 == 0: whole 16-byte pieces, 16-byte aligned.  The host keeps rows x pieces of one launch
// below 2^31 (compact_chunk_rows), so the index arithmetic is 32-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mi {

constexpr int COMPACT_THREADS = 256;
typedef float compact_v4f __attribute__((ext_vector_type(4)));

// out[i] = the source row of destination row first + i, i < n: compact_src (compact_host.h) per thread over the ascending
// list of deleted rows
__global__ __launch_bounds__(COMPACT_THREADS) void compact_src_kernel(const uint32_t* __restrict__ dead, uint32_t n_dead, uint32_t first,
                                                                      uint32_t n, uint32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * COMPACT_THREADS + threadIdx.x; i < n; i += gridDim.x * COMPACT_THREADS) {
        const uint32_t j = first + i;
        uint32_t lo = 0, hi = n_dead;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (dead[mid] - mid > j) hi = mid;
            else lo = mid + 1;
        }
        out[i] = j + lo;
    }
}

// dst row r (of n_rows, `pieces` 16-byte pieces each) = src row (rows ? rows[r] : r).  dst and src never overlap in the rows a
// launch touches (see above), so no __restrict__ promise beyond that is made.
__global__ __launch_bounds__(COMPACT_THREADS) void compact_move_kernel(const compact_v4f* src, compact_v4f* dst, const uint32_t* __restrict__ rows,
                                                                       uint32_t n_rows, uint32_t pieces) {
    const uint32_t total = n_rows * pieces;   // < 2^31: checked by the launcher
    for (uint32_t i = blockIdx.x * COMPACT_THREADS + threadIdx.x; i < total; i += gridDim.x * COMPACT_THREADS) {
        const uint32_t r = i / pieces, p = i - r * pieces;
        const uint32_t s = rows ? rows[r] : r;
        const compact_v4f v = __builtin_nontemporal_load(src + (size_t)s * pieces + p);
        __builtin_nontemporal_store(v, dst + i);
    }
}

// a column out of place: tmp[i] = col[rows[i]], i < n (the group column: 4-byte words; tags and stamps: 8-byte words)
template <class T>
__global__ __launch_bounds__(COMPACT_THREADS) void compact_gather_kernel(const T* __restrict__ col, const uint32_t* __restrict__ rows, uint32_t n,
                                                                         T* __restrict__ tmp) {
    for (uint32_t i = blockIdx.x * COMPACT_THREADS + threadIdx.x; i < n; i += gridDim.x * COMPACT_THREADS) tmp[i] = col[rows[i]];
}

}  // namespace mi
