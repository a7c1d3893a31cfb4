// compound_kernels.h — device code of mi_knn_search_compound: all-of / any-of / none-of terms in one pass over the fp32 rows.
//
// Every row gets the distance to EVERY term before anything is selected, each with the bits mi_knn_search(q = term) reports
// for it (the four fmaf chains, row16_sum and the distance expression of knn_scan_kernel).  The combination is done on the
// 32-bit distance KEYS (dist_to_u32), not on floats: the key order is the contract's order — numeric, -0 before +0, every
// NaN last and equal — so "largest / smallest under that order" is one unsigned max / min per term, a NaN term makes an ALL
// score NaN and drops out of an ANY score without a branch, and the score carries the bits of the term that decides it.
// Negative terms are tested on the floats (d <= within: a NaN never excludes).  A row then has ONE key to offer, and the
// selection is the search's own: per-wave register lists + knn_merge_kernel for k <= 64, one 32-bit key per row + the
// radix select (knn_select_*) above.
#pragma once
#include "../../include/mi355clip.h"
#include "knn_shared.h"

namespace mi {

constexpr int COMPOUND_MAX_TERMS = 8;
constexpr int COMPOUND_ALL = 0, COMPOUND_ANY = 1;

// run-time roles of the NT resident terms: bit u of neg_mask = term u is a negative one (excludes at d <= within[u]); the
// others are positive (the padding repeats the first positive term: it changes no max and no min)
struct CompoundTerms {
    uint32_t neg_mask;
    int mode;
    float within[COMPOUND_MAX_TERMS];
};

// The geometry of knn_scan_batched_kernel: a wave owns a tile of 64 rows, the 16-lane group g streams row 16 g + it with
// f32x4 nt loads, the NT terms sit in LDS and are read per use; after the 16 steps lane L holds the NT dots and x.x of
// its row.  grid: any number of 256-thread blocks, wave w of the grid takes tiles w, w + W, ...
//   list == nullptr: the tiles of the table (n = its rows); tomb (nullable) = the deletion bitmap, one word per tile.
//   list != nullptr: a tile = 64 consecutive entries of the ascending list of live local rows (n = its length), as
//                    knn_scan_gather_batched_kernel; entries past n repeat the last entry's row.
//   all_keys == nullptr: make_key(score, row) into one WaveTopReg per wave, stored to cand[wave][k] (k <= 64).
//   all_keys != nullptr: the row's (the entry's) 32-bit score key to all_keys[r] for the radix select.
// Excluded, deleted, out-of-range and NaN-score rows offer KEY_MAX (key word 0xFFFFFFFF).
// counts[0] += live candidates a negative term excluded, counts[1] += live candidates, not excluded, with a NaN score.
// Two waves per SIMD where the variant fits 256 registers without scratch (the batched search's 2 and 4 query forms run at two);
// 8 terms, and 4 at dim 1024, take one wave's worth, as knn_scan_batched_kernel<12, 8> does.
template <int NCH, int NT>
__global__ __launch_bounds__(256, (NT == 8 || (NT == 4 && NCH == 16)) ? 1 : 2) void knn_compound_scan_kernel(const float* __restrict__ table, uint64_t n,
                                                                const uint32_t* __restrict__ list,
                                                                const uint64_t* __restrict__ tomb,
                                                                const float* __restrict__ terms /*[NT][dim]*/, CompoundTerms ct,
                                                                uint32_t k, uint64_t* __restrict__ cand,
                                                                uint32_t* __restrict__ all_keys,
                                                                unsigned long long* __restrict__ counts) {
    constexpr int DIM = NCH * 64;
    __shared__ __attribute__((aligned(16))) float qs[NT * DIM];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const uint32_t wave = blockIdx.x * 4 + wib, n_waves = gridDim.x * 4;
    for (int j = threadIdx.x; j < NT * DIM; j += 256) qs[j] = terms[j];
    __syncthreads();

    float sq[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(&qs[u * DIM + 64 * t + 4 * i]);
            a.step(v, v);
        }
        sq[u] = sqrtf(a.sumsq());
    }
    WaveTopReg top;
    top.init(nullptr, k, lane);
    uint32_t n_excl = 0, n_nan = 0;

    const uint64_t n_tiles = (n + 63) >> 6;
    for (uint64_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint64_t e = (tile << 6) + lane;   // this lane's row (table form) or list entry
        uint32_t myrow = (uint32_t)e;
        if (list) myrow = list[e < n ? e : n - 1];
        uint64_t dead_w = 0;
        if (tomb && !list) dead_w = tomb[tile];
        float mydot[NT], myxx = 1.0f;
#pragma unroll
        for (int u = 0; u < NT; ++u) mydot[u] = 0.0f;
        const uint64_t row0 = (tile << 6) + 16 * g;
        for (int it = 0; it < 16; ++it) {
            uint64_t r = row0 + it;
            r = r < n ? r : n - 1;
            if (list) r = (uint32_t)__shfl((int)myrow, 16 * g + it, 64);
            const f32x4* p = reinterpret_cast<const f32x4*>(table + r * DIM) + i;
            f32x4 x[NCH];
#pragma unroll
            for (int t = 0; t < NCH; ++t) x[t] = __builtin_nontemporal_load(p + 16 * t);
            float s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                s0 = __builtin_fmaf(x[t].x, x[t].x, s0); s1 = __builtin_fmaf(x[t].y, x[t].y, s1);
                s2 = __builtin_fmaf(x[t].z, x[t].z, s2); s3 = __builtin_fmaf(x[t].w, x[t].w, s3);
            }
            const float s = row16_sum((s0 + s1) + (s2 + s3));
            if (i == it) myxx = s;
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                float d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
                for (int t = 0; t < NCH; ++t) {
                    // volatile: an LDS read per use, as in knn_scan_batched_kernel (hoisted, the NT x NCH fragments would
                    // need NT * 4 * NCH registers)
                    const f32x4 v = *reinterpret_cast<const volatile f32x4*>(&qs[u * DIM + 64 * t + 4 * i]);
                    d0 = __builtin_fmaf(v.x, x[t].x, d0); d1 = __builtin_fmaf(v.y, x[t].y, d1);
                    d2 = __builtin_fmaf(v.z, x[t].z, d2); d3 = __builtin_fmaf(v.w, x[t].w, d3);
                }
                const float d = row16_sum((d0 + d1) + (d2 + d3));
                if (i == it) mydot[u] = d;
            }
        }
        const float sx = sqrtf(myxx);
        uint32_t score = ct.mode == COMPOUND_ANY ? 0xFFFFFFFFu : 0u;
        bool excluded = false;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const float dist = 1.0f - mydot[u] / (sq[u] * sx);
            const uint32_t key = dist_to_u32(dist);
            if ((ct.neg_mask >> u) & 1u) excluded |= dist <= ct.within[u];
            else score = ct.mode == COMPOUND_ANY ? min(score, key) : max(score, key);
        }
        const bool live = e < n && !((dead_w >> lane) & 1ull);
        const bool nan = score == 0xFFFFFFFFu;
        n_excl += (uint32_t)__popcll(__ballot(live && excluded));
        n_nan += (uint32_t)__popcll(__ballot(live && !excluded && nan));
        const bool ok = live && !excluded && !nan;
        if (all_keys) {
            if (e < n) all_keys[e] = ok ? score : 0xFFFFFFFFu;
        } else {
            top.offer(ok ? (((uint64_t)score << 32) | myrow) : KEY_MAX);
        }
    }
    if (lane == 0) {
        if (n_excl) atomicAdd(&counts[0], (unsigned long long)n_excl);
        if (n_nan) atomicAdd(&counts[1], (unsigned long long)n_nan);
    }
    if (!all_keys) top.store(cand + (size_t)wave * k);
}

// The k sorted keys (score key << 32 | local row, ascending) -> idx / dist / term_dist, and the last two stats words.
// A key whose distance word is 0xFFFFFFFF is padding (this is where it differs from knn_finalize_kernel: the select path
// ranks excluded and NaN-score rows last, it does not drop them).  One 16-lane group per (result, term) recomputes d_j with
// RowAcc, exactly as knn_rescore_kernel does; the group of term 0 also writes the result's id and score.
// term_dist (nullable): [k][T].  stats[3] = results written (keys == nullptr: an empty candidate set, all padding).
template <int NCH>
__global__ __launch_bounds__(256) void knn_compound_finish_kernel(const float* __restrict__ table, const uint64_t* __restrict__ keys,
                                                                  uint32_t k, const float* __restrict__ terms, uint32_t T, IdMap map,
                                                                  uint64_t* __restrict__ idx, float* __restrict__ dist,
                                                                  float* __restrict__ term_dist, unsigned long long* __restrict__ stats) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t Tg = term_dist ? T : 1u;   // groups per result
    const uint32_t n_items = k * Tg;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    const float inf = __uint_as_float(0x7F800000u);
    // (whole 16-lane groups stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t c0 = group; c0 < ((n_items + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < n_items;
        const uint32_t j = live ? c0 / Tg : 0u, u = live ? c0 % Tg : 0u;
        const uint64_t key = keys ? keys[j] : KEY_MAX;
        const bool hit = (uint32_t)(key >> 32) != 0xFFFFFFFFu;
        const uint32_t row = hit ? (uint32_t)key : 0u;
        float d = inf;
        if (term_dist) {   // (uniform)
            const f32x4* p = reinterpret_cast<const f32x4*>(table + (uint64_t)row * DIM) + i;
            const f32x4* q = reinterpret_cast<const f32x4*>(terms + (size_t)u * DIM) + i;
            RowAcc<NCH> a, b; a.zero(); b.zero();
#pragma unroll
            for (int t = 0; t < NCH; ++t) {
                const f32x4 qv = q[16 * t];
                a.step(qv, p[16 * t]);
                b.step(qv, qv);
            }
            const float dot = a.dot(), s = a.sumsq(), sq = sqrtf(b.sumsq());
            if (hit) d = 1.0f - dot / (sq * sqrtf(s));
        }
        if (!live || i != 0) continue;
        if (term_dist) term_dist[(size_t)j * T + u] = d;
        if (u == 0) {
            idx[j] = hit ? id_of_local(map, (uint32_t)key) : MI_KNN_NO_ID;
            dist[j] = hit ? u32_to_dist((uint32_t)(key >> 32)) : inf;
            // the keys ascend: the hits are a prefix, its last entry knows the count
            const bool next_hit = j + 1 < k && keys && (uint32_t)(keys[j + 1] >> 32) != 0xFFFFFFFFu;
            if (hit && !next_hit) stats[3] = j + 1;
            if (!hit && j == 0) stats[3] = 0;
        }
    }
}

}  // namespace mi
