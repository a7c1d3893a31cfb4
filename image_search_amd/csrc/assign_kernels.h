// assign_kernels.h — device code of mi_knn_assign (every row of the table labelled by the nearest of C vectors) and of the
// update step of mi_knn_kmeans.
//
// The assign is the search turned round — not "the k rows nearest to a query" but "the 1 vector of C nearest to each of N
// rows" — in the two stages of the join (join_kernels.h): a first stage on the matrix pipe that may only err on the side
// of MORE candidates, and the fp32 arithmetic of knn_scan_kernel deciding.
//
// Stage 1 (assign_tiles_kernel).  A = the rows' bf16 mirror, B = the C vectors rounded by the same knn_mirror_kernel (so
// the marking of rows the bound does not cover comes with it).  A workgroup of four waves owns 128 table rows and walks
// the column tiles of 128 vectors; a tile is the join's: a wave a 64 x 64 quadrant as 2 x 2 accumulators of
// v_mfma_f32_32x32x16_bf16, K in steps of 64 through a double-buffered LDS image.  Per row it keeps a RUNNING maximum m of
// the normalised coarse cosine over the columns seen so far (an ordered-integer ds_max per row in LDS, after every tile)
// and emits (row, label) whenever  coarse >= m - 2 eps2.
//
// Why that is a superset.  eps2 is the join's, unchanged (both operands rounded to bf16: join_kernels.h,
//     eps2 = 2^-7 + 2^-16 + 4.1 (dim + 8) 2^-24 + 2e-6),
// |coarse(c) - exact(c)| <= eps2 for every pair the mirror does not mark.  Let c* be the vector the exact arithmetic
// prefers.  For every c:  coarse(c*) >= exact(c*) - eps2 >= exact(c) - eps2 >= coarse(c) - 2 eps2,  so c* passes against ANY
// m that is the coarse value of some column — in particular the running maximum, whatever the visiting order, and the
// maximum of a piece that sees only some of the columns (the overflow scheme of the host splits columns too; stage 2's
// per-row minimum joins the pieces).  A running maximum emits more than a final one would (the columns that led for a
// while); a first pass for the maximum and a second for the candidates would emit the final band only at twice the MFMA
// work.  The running form was kept: see DESIGN.md 5.16.
// The comparison is division-free per element: with w_a, w_b the square roots of the stored norms, the kernel compares
// v = acc * (1 / w_b)  (= w_a * coarse)  against  m_v - 2 eps2 * w_a — a reciprocal and a product, two roundings of relative
// 2^-24 on a quantity of magnitude <= w_a, 1.2e-7 on the cosine, inside the 2e-6 of eps2 (as the join's epilogue).
// Marked rows / vectors (norm stored as -1) are candidates against everything that is there and take no part in the
// maximum; deleted rows, rows beyond the table and the padding columns of the last tile never are.
//
// Stage 2 (assign_rescore_kernel): join_rescore_kernel's arithmetic per candidate — the table row is the QUERY (its
// sqrt(q.q) from RowAcc), the vector is the streamed row: dist = 1 - dot / (sq * sqrt(xx)), the bits mi_knn_search over a
// table of the vectors reports — then a 64-bit atomicMin per row on (dist_to_u32(dist) << 32 | label): the search's own
// order (distance ascending, then id, NaN last), independent of the arrival order.  assign_finalize_kernel unpacks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "tile128.h"

// (assign.hip and summary.hip both include this file: the kernels that are no templates are static, one copy per translation
// unit)
namespace mi {

constexpr int ASG_LDS = TILE_IMGS + 3 * TILE * 4;               // the tile's images + row weights, column weights, row maxima

// grid.x = row tiles: workgroup x takes rows of tile br0 + x against the column tiles [bc0, bc1).  thr = 2 eps2.
// count: all candidates found, also those beyond cap (the caller then redoes the piece in smaller ones); cand: the first
// `cap` of them as (row, label).
template <int NCH>
__global__ __launch_bounds__(256) void assign_tiles_kernel(const uint16_t* __restrict__ mirror, const float* __restrict__ xx,
                                                            const uint64_t* __restrict__ tomb, uint32_t n_rows,
                                                            const uint16_t* __restrict__ vmirror, const float* __restrict__ vxx,
                                                            uint32_t n_vec, uint32_t br0, uint32_t bc0, uint32_t bc1, float thr,
                                                            uint32_t cap, uint2* __restrict__ cand,
                                                            unsigned long long* __restrict__ count) {
    constexpr int DIM = NCH * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const TileFrag f = tile_frag();
    const int wr = f.wr, wc = f.wc, l31 = f.l31, lh = f.lh;
    // weights: rows  > 0 = sqrt of the stored norm, -1 = marked, 0 = not there;  columns  > 0 = 1 / sqrt(norm), -1, 0
    float* roww = reinterpret_cast<float*>(smem + TILE_IMGS);
    float* colw = roww + TILE;
    int* rowmax = reinterpret_cast<int*>(colw + TILE);
    const uint32_t row0 = (br0 + blockIdx.x) * TILE;

    if (tid < TILE) {
        const uint32_t r = row0 + (uint32_t)tid;
        roww[tid] = tile_weight<false>(xx, r, r < n_rows, tomb, r, -1.0f, 0.0f);
        rowmax[tid] = TILE_ORD_NINF;
    }
    const uint16_t *ga[4], *gb[4];
    tile_src<DIM>(ga, mirror, row0, n_rows);

#pragma unroll 1
    for (uint32_t bj = bc0; bj < bc1; ++bj) {
        const uint32_t col0 = bj * TILE;
        // (the previous tile's readers of colw and of the images passed the barrier that ends this iteration)
        if (tid < TILE) {
            const uint32_t cidx = col0 + (uint32_t)tid;
            colw[tid] = tile_weight<true>(vxx, cidx, cidx < n_vec, nullptr, 0u, -1.0f, 0.0f);
        }
        tile_src<DIM>(gb, vmirror, col0, n_vec);
        f32x16 acc[2][2];
        tile_accumulate<NCH>(smem, f, ga, gb, acc);

        // C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
        const float cw0 = colw[wc * 64 + l31], cw1 = colw[wc * 64 + 32 + l31];
        // (a) the tile's columns into the rows' running maxima
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ra0 = wr * 64 + ti * 32 + 8 * q + 4 * lh;
                const f32x4 wa = *reinterpret_cast<const f32x4*>(roww + ra0);
                const i32x4 mo = *reinterpret_cast<const i32x4*>(rowmax + ra0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float best = -__uint_as_float(0x7F800000u);
                    if (cw0 > 0.0f) best = fmaxf(best, acc[ti][0][4 * q + j] * cw0);
                    if (cw1 > 0.0f) best = fmaxf(best, acc[ti][1][4 * q + j] * cw1);
                    const int ob = tile_ord(best);
                    if (wa[j] > 0.0f && ob > mo[j]) atomicMax(rowmax + ra0 + j, ob);
                }
            }
        }
        __syncthreads();
        // (b) what the maxima cannot exclude
        unsigned long long hit = 0ull;   // bit (2 ti + tj) * 16 + e
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ra0 = wr * 64 + ti * 32 + 8 * q + 4 * lh;
                const f32x4 wa = *reinterpret_cast<const f32x4*>(roww + ra0);
                const i32x4 mo = *reinterpret_cast<const i32x4*>(rowmax + ra0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float bound = tile_unord(mo[j]) - thr * wa[j];
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) {
                        const float cw = tj ? cw1 : cw0;
                        const bool there = wa[j] != 0.0f && cw != 0.0f;
                        const bool ok = there && (wa[j] < 0.0f || cw < 0.0f || !(acc[ti][tj][4 * q + j] * cw < bound));
                        if (ok) hit |= 1ull << ((2 * ti + tj) * 16 + 4 * q + j);
                    }
                }
            }
        }
        tile_append(hit, f, row0, col0, cap, cand, count);
        __syncthreads();   // colw and the images may be overwritten
    }
}

// stage 2: n candidates (row, label) -> best[row] = min over them of (distance key << 32 | label)
template <int NCH>
__global__ __launch_bounds__(256) void assign_rescore_kernel(const float* __restrict__ table, const float* __restrict__ vec,
                                                             const uint2* __restrict__ cand, uint32_t n,
                                                             unsigned long long* __restrict__ best) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum is a cross-lane operation)
    for (uint32_t c0 = group; c0 < ((n + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < n;
        const uint2 pr = cand[live ? c0 : 0];
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)pr.x * DIM) + i;
        const f32x4* pb = reinterpret_cast<const f32x4*>(vec + (uint64_t)pr.y * DIM) + i;
        f32x4 qf[NCH];
#pragma unroll
        for (int t = 0; t < NCH; ++t) qf[t] = pa[16 * t];
        float sq;  // sqrt(q.q), same summation order as a row
        {
            RowAcc<NCH> a; a.zero();
#pragma unroll
            for (int t = 0; t < NCH; ++t) a.step(qf[t], qf[t]);
            sq = sqrtf(a.sumsq());
        }
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) a.step(qf[t], pb[16 * t]);
        const float d = a.dot(), s = a.sumsq();
        const float dist = 1.0f - d / (sq * sqrtf(s));
        if (live && i == 0) atomicMin(best + pr.x, (unsigned long long)make_key(dist, pr.y));
    }
}

// best -> labels / dist (deleted rows: MI_KNN_NO_LABEL, +inf).  prev (nullable): the previous assign's labels, the rows
// that differ are counted into *changed (an integer count: the same whatever the order).  prev may be `labels` itself.
static __global__ __launch_bounds__(256) void assign_finalize_kernel(const unsigned long long* __restrict__ best,
                                                                     const uint64_t* __restrict__ tomb, uint32_t n_rows,
                                                                     const uint32_t* prev, uint32_t* labels, float* __restrict__ dist,
                                                                     unsigned long long* __restrict__ changed) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    bool diff = false;
    if (r < n_rows) {
        const bool dead = tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull);
        const unsigned long long key = best[r];
        uint32_t lab = MI_KNN_NO_LABEL;
        float d = __uint_as_float(0x7F800000u);
        if (!dead && key != KEY_MAX) {
            lab = (uint32_t)key;
            d = u32_to_dist((uint32_t)(key >> 32));
        }
        if (prev) diff = prev[r] != lab;
        labels[r] = lab;
        dist[r] = d;
    }
    if (prev) {
        const unsigned long long m = __ballot(diff);
        if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(changed, (unsigned long long)__popcll(m));
    }
}

// ---- the update of mi_knn_kmeans ---------------------------------------------------------------------------------
// centroid[c] = (sum of x / |x| over the live rows labelled c whose distance is a number) / n_c, summed in an order the
// row ids fix: the rows are bucketed by label with a STABLE counting sort (members of a cluster ascending by row), a
// cluster's members are cut into segments of KM_SEG, a workgroup sums one segment (wave w the members w, w + 4, ... in
// order, the four waves combined as (0 + 1) + (2 + 3)), and the segments of a cluster are added in order.  No float
// atomics anywhere; the integer ones (histogram counts) give the same result in any order.
constexpr int KM_SEG = 512;

// 1 / |x| per row, the norm summed as the scan sums it
template <int NCH>
__global__ __launch_bounds__(256) void km_inv_norm_kernel(const float* __restrict__ table, uint32_t n_rows, float* __restrict__ inv) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    for (uint32_t r0 = group; r0 < ((n_rows + n_groups - 1) / n_groups) * n_groups; r0 += n_groups) {
        const bool live = r0 < n_rows;
        const uint32_t r = live ? r0 : n_rows - 1;
        const f32x4* p = reinterpret_cast<const f32x4*>(table + (uint64_t)r * DIM) + i;
        RowAcc<NCH> a; a.zero();
#pragma unroll
        for (int t = 0; t < NCH; ++t) { const f32x4 v = p[16 * t]; a.step(v, v); }
        const float s = a.sumsq();
        if (live && i == 0) inv[r] = 1.0f / sqrtf(s);
    }
}

// a row's bucket: its label, or C for the rows that feed no centroid (deleted, NaN distance)
__device__ __forceinline__ uint32_t km_bucket(const uint32_t* __restrict__ labels, const float* __restrict__ dist, uint32_t r, uint32_t C) {
    const uint32_t l = labels[r];
    const float d = dist[r];
    return (l >= C || d != d) ? C : l;
}

// wave w of the grid owns rows [w * chunk, (w + 1) * chunk) and the counters hist[w][0 .. C]
static __global__ __launch_bounds__(256) void km_hist_kernel(const uint32_t* __restrict__ labels, const float* __restrict__ dist,
                                                             uint32_t n_rows, uint32_t C, uint32_t chunk, uint32_t* __restrict__ hist) {
    const uint32_t w = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const uint64_t lo = (uint64_t)w * chunk, hi = lo + chunk < n_rows ? lo + chunk : n_rows;
    uint32_t* h = hist + (size_t)w * (C + 1);
    for (uint64_t r = lo + lane; r < hi; r += 64) atomicAdd(h + km_bucket(labels, dist, (uint32_t)r, C), 1u);
}

// per bucket: hist[w][c] -> the number of members in the chunks before w; total[c] = all of them
static __global__ __launch_bounds__(256) void km_scan_kernel(uint32_t* __restrict__ hist, uint32_t n_waves, uint32_t C,
                                                             uint32_t* __restrict__ total) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c > C) return;
    uint32_t run = 0;
    for (uint32_t w = 0; w < n_waves; ++w) {
        const uint32_t t = hist[(size_t)w * (C + 1) + c];
        hist[(size_t)w * (C + 1) + c] = run;
        run += t;
    }
    total[c] = run;
}

// one workgroup: start[c] = members in the buckets before c (start[C + 1] = all rows), seg[c] = segments of the clusters
// before c (seg[C] = all segments; the bucket C has none)
static __global__ __launch_bounds__(1024) void km_offsets_kernel(const uint32_t* __restrict__ total, uint32_t C, uint32_t* __restrict__ start,
                                                                 uint32_t* __restrict__ seg) {
    __shared__ uint32_t s_rows[1024], s_segs[1024];
    const uint32_t n = C + 1, per = (n + 1023) / 1024, t = threadIdx.x;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t rows = 0, segs = 0;
    for (uint32_t c = lo; c < hi; ++c) { rows += total[c]; if (c < C) segs += (total[c] + KM_SEG - 1) / KM_SEG; }
    s_rows[t] = rows; s_segs[t] = segs;
    __syncthreads();
    if (t == 0) {
        uint32_t r = 0, s = 0;
        for (int u = 0; u < 1024; ++u) { const uint32_t a = s_rows[u], b = s_segs[u]; s_rows[u] = r; s_segs[u] = s; r += a; s += b; }
    }
    __syncthreads();
    rows = s_rows[t]; segs = s_segs[t];
    for (uint32_t c = lo; c < hi; ++c) {
        start[c] = rows; seg[c] = segs;
        rows += total[c];
        if (c < C) segs += (total[c] + KM_SEG - 1) / KM_SEG;
    }
    if (hi == n && lo < n) { start[n] = rows; }
    if (hi == n && lo < n) seg[n] = segs;
}

// the stable placement: wave w walks its rows 64 at a time in order; the lanes of one bucket take consecutive slots in
// lane order.  Lane 0 alone reads and advances the wave's counters (one thread, program order).
static __global__ __launch_bounds__(256) void km_place_kernel(const uint32_t* __restrict__ labels, const float* __restrict__ dist,
                                                              uint32_t n_rows, uint32_t C, uint32_t chunk, uint32_t* hist,
                                                              const uint32_t* __restrict__ start, uint32_t* __restrict__ sorted) {
    const uint32_t w = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const uint64_t lo = (uint64_t)w * chunk, hi = lo + chunk < n_rows ? lo + chunk : n_rows;
    uint32_t* h = hist + (size_t)w * (C + 1);
    for (uint64_t r0 = lo; r0 < hi; r0 += 64) {
        const uint64_t r = r0 + lane;
        bool todo = r < hi;
        const uint32_t b = todo ? km_bucket(labels, dist, (uint32_t)r, C) : 0u;
        unsigned long long left = __ballot(todo);
        while (left) {
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t b0 = (uint32_t)__shfl((int)b, leader, 64);
            const unsigned long long m = __ballot(todo && b == b0);
            uint32_t base = 0;
            if (lane == 0) {
                base = h[b0];
                h[b0] = base + (uint32_t)__popcll(m);
            }
            base = (uint32_t)__shfl((int)base, 0, 64);
            if (todo && b == b0) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                sorted[start[b0] + base + rank] = (uint32_t)r;
                todo = false;
            }
            left &= ~m;
        }
    }
}

// workgroup g = segment g (of cluster c: seg[c] <= g < seg[c + 1]) -> part[g][dim]
template <int NCH>
__global__ __launch_bounds__(256) void km_sum_kernel(const float* __restrict__ table, const float* __restrict__ inv,
                                                     const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ start,
                                                     const uint32_t* __restrict__ seg, uint32_t C, float* __restrict__ part) {
    constexpr int DIM = NCH * 64, NT = (DIM + 255) / 256;
    __shared__ __attribute__((aligned(16))) float sh[4][NT * 256];
    const uint32_t g = blockIdx.x;
    if (g >= seg[C]) return;
    uint32_t lo = 0, hi = C;   // the last c with seg[c] <= g
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t first = start[c] + (g - seg[c]) * KM_SEG;
    const uint32_t n = min((uint32_t)KM_SEG, start[c + 1] - first);
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (uint32_t m = wib; m < n; m += 4) {
        const uint32_t r = sorted[first + m];
        const float s = inv[r];
        const f32x4* p = reinterpret_cast<const f32x4*>(table + (uint64_t)r * DIM) + lane;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (4 * lane + 256 * t < DIM) acc[t] += p[64 * t] * s;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(&sh[wib][256 * t + 4 * lane]) = acc[t];
    __syncthreads();
    for (int j = threadIdx.x; j < DIM; j += 256) part[(size_t)g * DIM + j] = (sh[0][j] + sh[1][j]) + (sh[2][j] + sh[3][j]);
}

// thread (c, j): the cluster's segments in order, divided by its size; an empty cluster keeps its centroid
static __global__ __launch_bounds__(256) void km_centroid_kernel(const float* __restrict__ part, const uint32_t* __restrict__ total,
                                                                 const uint32_t* __restrict__ seg, uint32_t C, uint32_t dim,
                                                                 float* __restrict__ centroids) {
    const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (uint64_t)C * dim) return;
    const uint32_t c = (uint32_t)(at / dim), j = (uint32_t)(at % dim);
    const uint32_t n = total[c];
    if (n == 0) return;
    float s = 0.0f;
    for (uint32_t g = seg[c]; g < seg[c + 1]; ++g) s += part[(size_t)g * dim + j];
    centroids[at] = s / (float)n;
}

// ---- the same update on exact integer sums (option "kmeans_fixed_sum"; always across shards) ---------------------------
// A member row r adds q = (|v| < 2) ? rint(v * 2^30) : 0 per component, v = x[r][j] * inv[r] (the float path's product;
// the scaling is exact, the rounding to nearest even, a NaN or inf v fails the comparison), into a 64-bit sum: |q| < 2^31
// and fewer than 2^32 members keep |S| < 2^63.  Integer sums are the same in any order, so the segments, the waves of a
// segment and the shards of a table may be added as they come; centroid = (float)((double)S * 2^-30 / (double)n).  The
// rules restated for the host: kmeans_fixed_host.h.
__device__ __forceinline__ long long km_quant(float v) {
    return fabsf(v) < 2.0f ? (long long)(int)rintf(v * 0x1p30f) : 0ll;   // |rint| <= 2^31 - 128: it fits 32 bits
}

// workgroup g = segment g, as in km_sum_kernel -> ipart[g][dim]; a thread keeps 4 * NT 64-bit sums
template <int NCH>
__global__ __launch_bounds__(256) void km_sum_fixed_kernel(const float* __restrict__ table, const float* __restrict__ inv,
                                                           const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ start,
                                                           const uint32_t* __restrict__ seg, uint32_t C, long long* __restrict__ ipart) {
    constexpr int DIM = NCH * 64, NT = (DIM + 255) / 256;
    __shared__ __attribute__((aligned(16))) long long sh[3][NT * 256];   // waves 1 .. 3; wave 0 adds from its registers
    const uint32_t g = blockIdx.x;
    if (g >= seg[C]) return;
    uint32_t lo = 0, hi = C;   // the last c with seg[c] <= g
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t first = start[c] + (g - seg[c]) * KM_SEG;
    const uint32_t n = min((uint32_t)KM_SEG, start[c + 1] - first);
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    long long acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0;
#pragma unroll 4
    for (uint32_t m = wib; m < n; m += 4) {
        const uint32_t r = sorted[first + m];
        const float s = inv[r];
        const f32x4* p = reinterpret_cast<const f32x4*>(table + (uint64_t)r * DIM) + lane;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (4 * lane + 256 * t < DIM) {
                const f32x4 v = p[64 * t] * s;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][e] += km_quant(v[e]);
            }
    }
    if (wib != 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) sh[wib - 1][256 * t + 4 * lane + e] = acc[t][e];
    }
    __syncthreads();
    if (wib == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (4 * lane + 256 * t < DIM) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 256 * t + 4 * lane + e;
                    ipart[(size_t)g * DIM + j] = acc[t][e] + sh[0][j] + sh[1][j] + sh[2][j];
                }
            }
    }
}

// thread (c, j): S[c][j] = the cluster's segments added; thread (c, 0) writes n[c]
static __global__ __launch_bounds__(256) void km_reduce_fixed_kernel(const long long* __restrict__ ipart, const uint32_t* __restrict__ total,
                                                                     const uint32_t* __restrict__ seg, uint32_t C, uint32_t dim,
                                                                     long long* __restrict__ S, uint32_t* __restrict__ cnt) {
    const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (uint64_t)C * dim) return;
    const uint32_t c = (uint32_t)(at / dim), j = (uint32_t)(at % dim);
    long long s = 0;
    for (uint32_t g = seg[c]; g < seg[c + 1]; ++g) s += ipart[(size_t)g * dim + j];
    S[at] = s;
    if (j == 0) cnt[c] = total[c];
}

// another shard's sums and counts added into this one's: S[i] += S_in[i] for i < n_S, cnt[c] += cnt_in[c] for c < n_cnt
static __global__ __launch_bounds__(256) void km_merge_fixed_kernel(long long* __restrict__ S, const long long* __restrict__ S_in, uint64_t n_S,
                                                                    uint32_t* __restrict__ cnt, const uint32_t* __restrict__ cnt_in,
                                                                    uint32_t n_cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_S; i += stride) S[i] += S_in[i];
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < n_cnt; c += stride) cnt[c] += cnt_in[c];
}

// thread (c, j): the sum as a double, scaled back and divided by the cluster's size; an empty cluster keeps its centroid
static __global__ __launch_bounds__(256) void km_centroid_fixed_kernel(const long long* __restrict__ S, const uint32_t* __restrict__ cnt,
                                                                       uint32_t C, uint32_t dim, float* __restrict__ centroids) {
    const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (uint64_t)C * dim) return;
    const uint32_t n = cnt[at / dim];
    if (n == 0) return;
    centroids[at] = (float)((double)S[at] * 0x1p-30 / (double)n);
}

}  // namespace mi
