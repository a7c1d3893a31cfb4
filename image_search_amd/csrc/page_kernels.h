// page_kernels.h — device code of mi_knn_search_page: the k smallest of the search's 64-bit keys inside a window
// [first_key, hi], and how many candidates lie on either side of it, in one pass over the fp32 rows.
//
// A page is "the next k after a cursor, within a distance".  Both ends are applied to the KEYS (dist_to_u32(d) << 32 | local
// row), not to floats and not to ranks: the key order IS the result order (distance ascending, -0 before +0, id ascending
// among equal distances, every NaN last), a key is unique per row, so "key > cursor key" cuts a group of equal distances at the
// cursor's id and stays right when rows are appended or deleted between two pages; the bound compares distance words, which
// makes it inclusive under the same order.  The row's distance has the bits mi_knn_search reports: RowAcc, row16_sum and the
// distance expression of knn_scan_kernel, in its order.  Nothing is selected here that the search does not select already:
// per-wave register lists + knn_merge_kernel for k <= 64, one 32-bit key per row + the radix select (knn_select_*) above.
#pragma once
#include "../../include/mi355clip.h"
#include "knn_shared.h"

namespace mi {

// The geometry of knn_scan_kernel: a wave owns a tile of 64 rows, the 16-lane group g streams row 16 g + it with f32x4 nt
// loads, two row buffers in flight, the query in registers; after the 16 steps lane L holds q.x and x.x of its row.
// grid: any number of 256-thread blocks, wave w of the grid takes tiles w, w + W, ...
//   list == nullptr: the tiles of the table (n = its rows, n >= 1); tomb (nullable) = the deletion bitmap, one word per tile.
//   list != nullptr: a tile = 64 consecutive entries of the ascending list of live local rows (n = its length, n >= 1), as
//                    knn_scan_gather_kernel; entries past n repeat the last entry's row.
// A live candidate with key = make_key(dist, local row) falls in the first class that applies:
//   before  key < first_key          (first_key = 0: no cursor, nothing is before)
//   window  key <= hi                (hi = bound's distance word << 32 | 0xFFFFFFFF; a NaN distance word is above every hi)
//   beyond  the distance is not NaN
//   nan
// counted with ballots into four wave-uniform words, one atomic add per wave and non-zero class at the end.  Deleted and
// out-of-range lanes count nowhere.
//   KEYS == 0 (k <= 64): rows outside the window offer KEY_MAX to the wave's WaveTopReg, stored to cand[wave][k].
//   KEYS == 1: the row's (the entry's) 32-bit distance key to all_keys[r], 0xFFFFFFFF for everything outside the window —
//              equal-distance rows at or below the cursor's id included — for the radix select over (key, position).
template <int NCH, int KEYS>
__global__ __launch_bounds__(256, 2) void knn_page_scan_kernel(const float* __restrict__ table, uint64_t n,
                                                               const uint32_t* __restrict__ list,
                                                               const uint64_t* __restrict__ tomb, const float* __restrict__ q,
                                                               uint64_t first_key, uint64_t hi, uint32_t k,
                                                               uint64_t* __restrict__ cand, uint32_t* __restrict__ all_keys,
                                                               unsigned long long* __restrict__ counts) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const uint32_t wave = blockIdx.x * 4 + wib, n_waves = gridDim.x * 4;

    f32x4 qf[NCH];
#pragma unroll
    for (int t = 0; t < NCH; ++t) qf[t] = *reinterpret_cast<const f32x4*>(q + 64 * t + 4 * i);
    float sq;  // sqrt(q.q), same summation order as a row
    {
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
        sq = sqrtf(a.sumsq());
    }
    WaveTopReg top;
    top.init(nullptr, k, lane);
    uint32_t n_before = 0, n_window = 0, n_beyond = 0, n_nan = 0;

    const uint64_t n_tiles = (n + 63) >> 6;
    auto load_row = [&](f32x4 (&x)[NCH], uint64_t r) {
        const f32x4* p = reinterpret_cast<const f32x4*>(table + r * DIM) + i;
#pragma unroll
        for (int t = 0; t < NCH; ++t) x[t] = __builtin_nontemporal_load(p + 16 * t);
    };
    for (uint64_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint64_t e = (tile << 6) + lane;   // this lane's row (table form) or list entry
        uint32_t myrow = (uint32_t)e;
        if (list) myrow = list[e < n ? e : n - 1];
        const uint64_t row0 = (tile << 6) + 16 * g;
        // the row the group streams in step it: (wave-uniform choice of the source)
        auto row_at = [&](int it) -> uint64_t {
            if (list) return (uint32_t)__shfl((int)myrow, 16 * g + it, 64);
            const uint64_t r = row0 + it;
            return r < n ? r : n - 1;
        };
        float mydot = 0.0f, myxx = 1.0f;
        auto reduce_row = [&](const f32x4 (&x)[NCH], int it) {
            RowAcc<NCH> a; a.zero();
#pragma unroll
            for (int t = 0; t < NCH; ++t) a.step(qf[t], x[t]);
            const float d = a.dot(), s = a.sumsq();
            if (i == it) { mydot = d; myxx = s; }
        };
        f32x4 xa[NCH], xb[NCH];
        load_row(xa, row_at(0));
#pragma unroll 1
        for (int it = 0; it < 16; it += 2) {
            load_row(xb, row_at(it + 1));
            reduce_row(xa, it);
            load_row(xa, row_at(it + 2 < 16 ? it + 2 : 15));
            reduce_row(xb, it + 1);
        }
        uint64_t dead_w = 0;
        if (tomb && !list) dead_w = tomb[tile];
        const float dist = 1.0f - mydot / (sq * sqrtf(myxx));
        const uint32_t dk = dist_to_u32(dist);
        const uint64_t key = ((uint64_t)dk << 32) | myrow;
        const bool live = e < n && !((dead_w >> lane) & 1ull);
        const bool before = key < first_key;
        const bool in = live && !before && key <= hi;
        n_before += (uint32_t)__popcll(__ballot(live && before));
        n_window += (uint32_t)__popcll(__ballot(in));
        n_beyond += (uint32_t)__popcll(__ballot(live && !before && key > hi && dk != 0xFFFFFFFFu));
        n_nan += (uint32_t)__popcll(__ballot(live && !before && key > hi && dk == 0xFFFFFFFFu));
        if constexpr (KEYS == 1) {
            if (e < n) all_keys[e] = in ? dk : 0xFFFFFFFFu;
        } else {
            top.offer(in ? key : KEY_MAX);
        }
    }
    if (lane == 0) {
        if (n_before) atomicAdd(&counts[0], (unsigned long long)n_before);
        if (n_window) atomicAdd(&counts[1], (unsigned long long)n_window);
        if (n_beyond) atomicAdd(&counts[2], (unsigned long long)n_beyond);
        if (n_nan) atomicAdd(&counts[3], (unsigned long long)n_nan);
    }
    if constexpr (KEYS == 0) top.store(cand + (size_t)wave * k);
}

// The k sorted keys (distance key << 32 | local row, ascending) -> idx / dist; one thread per result slot.  A key whose
// distance word is 0xFFFFFFFF is padding (KEY_MAX from the lists; a row outside the window the select ranked last): no
// rescore is needed, a key maps back to one float.
__global__ void knn_page_finish_kernel(const uint64_t* __restrict__ keys, uint32_t k, IdMap map, uint64_t* __restrict__ idx,
                                       float* __restrict__ dist) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint64_t key = keys[j];
    const bool hit = (uint32_t)(key >> 32) != 0xFFFFFFFFu;
    idx[j] = hit ? id_of_local(map, (uint32_t)key) : MI_KNN_NO_ID;
    dist[j] = hit ? u32_to_dist((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
}

}  // namespace mi
