// knn_shared.h — the search's arithmetic that other translation units build on: the vector types, the 16-lane sum and
// RowAcc (the summation order that defines "the search's bits"), the 64-bit keys and the register form of the per-wave top-k
// (WaveTopReg), the bf16 mirror (knn_mirror_kernel) and
// the row ids of a shard (ids.h).  Everything here is a template or inline, so any number of translation units may include it;
// knn_kernels.h includes it and keeps the search's own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ids.h"

namespace mi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint64_t KEY_MAX = 0xFFFFFFFFFFFFFFFFull;

// ---- DPP helpers (16-lane rows) -------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// After the xor-1 and xor-2 steps the four lanes of a quad agree, so the half-mirror
// (lane -> 7-lane) delivers the other quad's sum = the xor-4 partner's; likewise the
// row mirror (lane -> 15-lane) is the xor-8 partner once the 8-lane halves agree.
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]  : xor 1
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]  : xor 2
    v += dpp_mov<0x141>(v);  // row_half_mirror      : xor 4
    v += dpp_mov<0x140>(v);  // row_mirror           : xor 8
    return v;
}

// ---- keys -----------------------------------------------------------------------
__device__ __forceinline__ uint32_t dist_to_u32(float d) {
    uint32_t b = __float_as_uint(d);
    if (d != d) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float u32_to_dist(uint32_t k) {
    if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ uint64_t make_key(float d, uint32_t row) {
    return ((uint64_t)dist_to_u32(d) << 32) | row;
}
// ---- 64-bit keys across lanes --------------------------------------------------------
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a < b ? b : a; }

// ---- per-wave top-k, register form (one key per lane) -----------------------------
struct WaveTopReg {
    static constexpr int KP = 64;
    static constexpr int LDS_KEYS = 0;
    uint64_t best, thr;
    uint32_t k;
    int lane;

    __device__ void init(uint64_t*, uint32_t k_, int lane_) {
        best = KEY_MAX; thr = KEY_MAX; k = k_; lane = lane_;
    }
    __device__ static uint64_t sort_asc(uint64_t v, int lane) {
#pragma unroll
        for (int kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
            for (int j = kk >> 1; j > 0; j >>= 1) {
                const uint64_t o = shfl_xor64(v, j);
                const bool up = (lane & kk) == 0, lower = (lane & j) == 0;
                v = (lower == up) ? umin64(v, o) : umax64(v, o);
            }
        }
        return v;
    }
    __device__ static uint64_t merge_bitonic(uint64_t v, int lane) {
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) {
            const uint64_t o = shfl_xor64(v, j);
            v = ((lane & j) == 0) ? umin64(v, o) : umax64(v, o);
        }
        return v;
    }
    // wave-collective: every lane offers one key (KEY_MAX = nothing)
    __device__ void offer(uint64_t key) {
        const bool pass = key < thr;
        if (__ballot(pass) == 0ull) return;
        uint64_t c = sort_asc(pass ? key : KEY_MAX, lane);
        c = shfl64(c, 63 - lane);
        best = merge_bitonic(umin64(best, c), lane);
        thr = shfl64(best, (int)k - 1);
    }
    __device__ void finish() {}
    // store the k best keys, ascending
    __device__ void store(uint64_t* out) const {
        if ((uint32_t)lane < k) out[lane] = best;
    }
    __device__ uint64_t lane_key(int) const { return best; }
};

// ---- the scan ---------------------------------------------------------------------
// One fp32 fmaf per (row element, accumulator); NCH = dim / 64 chunks of 256 bytes.
template <int NCH>
struct RowAcc {
    float d0, d1, d2, d3, s0, s1, s2, s3;
    __device__ __forceinline__ void zero() { d0 = d1 = d2 = d3 = s0 = s1 = s2 = s3 = 0.0f; }
    __device__ __forceinline__ void step(const f32x4& q, const f32x4& x) {
        d0 = __builtin_fmaf(q.x, x.x, d0); d1 = __builtin_fmaf(q.y, x.y, d1);
        d2 = __builtin_fmaf(q.z, x.z, d2); d3 = __builtin_fmaf(q.w, x.w, d3);
        s0 = __builtin_fmaf(x.x, x.x, s0); s1 = __builtin_fmaf(x.y, x.y, s1);
        s2 = __builtin_fmaf(x.z, x.z, s2); s3 = __builtin_fmaf(x.w, x.w, s3);
    }
    __device__ __forceinline__ float dot() const { return row16_sum((d0 + d1) + (d2 + d3)); }
    __device__ __forceinline__ float sumsq() const { return row16_sum((s0 + s1) + (s2 + s3)); }
};

// ---- the bf16 mirror (knn_kernels.h "bf16 mirror as prefilter") ---------------------------------------------------
constexpr uint32_t PREF_CAP = 1u << 22;  // candidates stage 2 accepts (4 M rows = 12.9 GB of fp32 rows at dim 768: two fifths of a 10 M-row pass)

// rows [first, end) of the table -> bf16 mirror rows + stored squared norms (-1 = "always a candidate")
template <int NCH>
__global__ __launch_bounds__(256) void knn_mirror_kernel(const float* __restrict__ table, uint64_t first, uint64_t end,
                                                         uint16_t* __restrict__ mirror, float* __restrict__ xx) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint64_t group = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = ((uint64_t)gridDim.x * 256) >> 4;
    for (uint64_t r0 = first + group; r0 < ((end - first + n_groups - 1) / n_groups) * n_groups + first; r0 += n_groups) {
        const bool live = r0 < end;  // (whole 16-lane groups stay in the loop: row16_sum is a cross-lane operation)
        const uint64_t r = live ? r0 : end - 1;
        const f32x4* p = reinterpret_cast<const f32x4*>(table + r * DIM) + i;
        float s = 0.0f;
        bool bad = false;
#pragma unroll
        for (int t = 0; t < NCH; ++t) {
            const f32x4 v = p[16 * t];
            const float e[4] = {v.x, v.y, v.z, v.w};
            uint32_t b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bad |= !(fabsf(e[j]) <= 3.0e38f);  // NaN, inf, and what bf16 would round to inf
                s = __builtin_fmaf(e[j], e[j], s);
                const uint32_t u = __float_as_uint(e[j]);
                b[j] = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;  // round to nearest even
            }
            if (live) *reinterpret_cast<uint2*>(mirror + r * DIM + 64 * t + 4 * i) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
        }
        s = row16_sum(s);
        const unsigned long long bm = __ballot(bad);
        const bool any_bad = ((bm >> (lane & 48)) & 0xFFFFull) != 0ull;
        if (live && i == 0) xx[r] = (any_bad || !(s >= 1.0e-30f && s <= 1.0e30f)) ? -1.0f : s;
    }
}

}  // namespace mi
