// tile128.h — the 128 x 128 bf16 tile that stage 1 of the threshold-pair calls (the join, the join of two row sets, the
// density passes: pair_kernels.h), the assign, the multi-label assign and the many-query search share (join_kernels.h has
// the bound eps2 that makes such a first stage exact; each kernel's header has its own superset
// argument).  S = A B^T over two bf16 mirrors (knn_mirror_kernel: rows rounded to nearest even, stored fp32 squared norms,
// -1 = marked).  A workgroup of four waves owns one tile, a wave a 64 x 64 quadrant as 2 x 2 accumulators of
// v_mfma_f32_32x32x16_bf16; K runs in steps of 64 elements through a double-buffered LDS image (2 x 2 x 16 KiB, at the
// start of the kernel's dynamic LDS).  A kernel decides which accumulators are candidates (its epilogue: the `hit` mask)
// and what it keeps per row beside them; the pieces here are the same for all:
//     tile_frag / tile_src    where a thread's loads come from and go to,
//     tile_accumulate         the K loop,
//     tile_weight             a row's weight from its stored norm,
//     tile_append             the `hit` mask -> the candidate buffer, one atomic per wave that has any.
// pair_tile (pair_kernels.h) puts the four together with the threshold test as its epilogue: the whole stage 1 of the
// threshold-pair calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "knn_shared.h"

namespace mi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 128;                                  // rows of a tile, both ways
constexpr int TILE_KC = 64;                                // elements of K per LDS image (128 bytes per row)
constexpr int TILE_IMG = TILE * TILE_KC * 2;               // bytes of one operand's image
constexpr int TILE_IMGS = 4 * TILE_IMG;                    // two buffers of two operands: what a kernel's own LDS follows
constexpr uint32_t TILE_CAP_MIN = TILE * TILE;             // a candidate buffer holds at least one full tile

// 16-byte chunk `ch` (0..7) of row `row` inside an operand image of 128-byte rows.  The xor spreads the 16 rows a
// ds_read_b128 serves at once (lanes l .. l + 15: consecutive rows, one chunk) over all 64 banks: even rows start in
// banks 0..31, odd rows in 32..63, and the 8 rows of either parity take 8 different chunks.
__device__ __forceinline__ uint32_t tile_lds_off(int row, int ch) { return (uint32_t)(row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)); }
// floats as integers of the same order (an involution), for ds_max_i32
__device__ __forceinline__ int tile_ord(float f) { const int b = __float_as_int(f); return b ^ ((b >> 31) & 0x7FFFFFFF); }
__device__ __forceinline__ float tile_unord(int o) { return __int_as_float(o ^ ((o >> 31) & 0x7FFFFFFF)); }
constexpr int TILE_ORD_NINF = (int)0x807FFFFFu;            // tile_ord(-inf): a running maximum nothing has entered

__device__ __forceinline__ bool tile_dead(const uint64_t* __restrict__ tomb, uint32_t r) { return tomb && ((tomb[r >> 6] >> (r & 63)) & 1ull); }

// The weight of row r of one side of a tile, from its stored norm xx[r]: sqrt (INV: 1 / sqrt); `marked` where the mirror
// marked the row (a candidate against everything that is there); `absent` where it is not `there` (beyond the table, the
// padding of the last tile) or deleted (bit tomb_r of tomb; tomb may be null).
template <bool INV>
__device__ __forceinline__ float tile_weight(const float* __restrict__ xx, uint32_t r, bool there, const uint64_t* __restrict__ tomb,
                                             uint32_t tomb_r, float marked, float absent) {
    float w = absent;
    if (there) {
        if (!tile_dead(tomb, tomb_r)) {
            const float s = xx[r];
            w = s < 0.0f ? marked : (INV ? 1.0f / sqrtf(s) : sqrtf(s));
        }
    }
    return w;
}

// A thread's fixed places in the tile.  global -> registers -> LDS: thread t moves chunk t & 7 of rows t >> 3, + 32, + 64,
// + 96 of both operands to lo[].  Operand lane map of the 32x32x16 form: lane (r = l & 31, h = l >> 5) holds elements
// k = 8 h .. 8 h + 7 of row r; fa / fb are the byte offsets of this lane's rows, the chunk xor applied per read.
struct TileFrag {
    uint32_t lo[4], fa[2], fb[2];
    int swz_a0, swz_b0, wr, wc, l31, lh;
};
__device__ __forceinline__ TileFrag tile_frag() {
    TileFrag f;
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    f.wr = wib >> 1; f.wc = wib & 1; f.l31 = lane & 31; f.lh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) f.lo[j] = tile_lds_off((tid >> 3) + 32 * j, tid & 7);
    f.swz_a0 = ((f.wr * 64 + f.l31) >> 1) & 7; f.swz_b0 = ((f.wc * 64 + f.l31) >> 1) & 7;   // (+ 32 rows: the same xor, 32 >> 1 = 16)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        f.fa[t] = (uint32_t)((f.wr * 64 + t * 32 + f.l31) * 128);
        f.fb[t] = (uint32_t)(TILE_IMG + (f.wc * 64 + t * 32 + f.l31) * 128);
    }
    return f;
}

// where this thread's four loads of one operand come from: rows row0 + (t >> 3) + 32 j of a mirror of n_rows rows
template <int DIM>
__device__ __forceinline__ void tile_src(const uint16_t* (&g)[4], const uint16_t* __restrict__ mirror, uint32_t row0, uint32_t n_rows) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (tid >> 3) + 32 * j, ch = tid & 7;
        const uint32_t r = min(row0 + (uint32_t)row, n_rows - 1);   // a ragged last tile rereads the last row
        g[j] = mirror + (size_t)r * DIM + ch * 8;
    }
}

// acc = A B^T over the whole K = NCH * 64 of the tile whose rows ga / gb point at.  All 256 threads call it; when it
// returns, every wave has passed the last barrier: the images (and whatever LDS the caller wrote before) may be reused.
template <int NCH>
__device__ __forceinline__ void tile_accumulate(unsigned char* smem, const TileFrag& f, const uint16_t* const (&ga)[4],
                                                const uint16_t* const (&gb)[4], f32x16 (&acc)[2][2]) {
    static_assert(NCH % 2 == 0, "rows of whole 256-byte bf16 chunks (the mirror's own condition)");
    constexpr int NK = NCH * 64 / TILE_KC;
    u32x4 sa[4], sb[4];   // (the native vector type: arrays of HIP's uint4 struct stayed in scratch memory)
    auto fetch = [&](int kc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sa[j] = *reinterpret_cast<const u32x4*>(ga[j] + kc * TILE_KC);
            sb[j] = *reinterpret_cast<const u32x4*>(gb[j] + kc * TILE_KC);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<u32x4*>(smem + buf * (2 * TILE_IMG) + f.lo[j]) = sa[j];
            *reinterpret_cast<u32x4*>(smem + buf * (2 * TILE_IMG) + TILE_IMG + f.lo[j]) = sb[j];
        }
    };
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ti][tj][e] = 0.0f;

    fetch(0);
    stash(0);
    __syncthreads();
#pragma unroll 1
    for (int kc = 0; kc < NK; ++kc) {
        if (kc + 1 < NK) fetch(kc + 1);
        const unsigned char* img = smem + (kc & 1) * (2 * TILE_IMG);
#pragma unroll
        for (int s = 0; s < TILE_KC / 16; ++s) {
            const int ch = 2 * s + f.lh;
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[t] = *reinterpret_cast<const bf16x8*>(img + f.fa[t] + ((ch ^ f.swz_a0) << 4));
                bf[t] = *reinterpret_cast<const bf16x8*>(img + f.fb[t] + ((ch ^ f.swz_b0) << 4));
            }
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
        }
        // the other buffer's last readers passed the barrier that ended the previous step
        if (kc + 1 < NK) stash((kc + 1) & 1);
        __syncthreads();
    }
}

// C/D map: register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block; bit
// (2 ti + tj) * 16 + e of `hit` marks accumulator acc[ti][tj][e] of this lane as a candidate.  The wave's candidates are
// appended as (row0 + row, col0 + column): a prefix sum over the lanes, one atomic per wave that has any.  count: all
// candidates found, also those beyond cap (the caller then redoes the piece in smaller ones); cand: the first `cap`.
__device__ __forceinline__ void tile_append(unsigned long long hit, const TileFrag& f, uint32_t row0, uint32_t col0, uint32_t cap,
                                            uint2* __restrict__ cand, unsigned long long* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const uint32_t mine = (uint32_t)__popcll(hit);
    if (__ballot(mine != 0u) == 0ull) return;   // what almost every tile of a real corpus does
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    unsigned long long base = 0ull;
    if (lane == 63) base = atomicAdd(count, (unsigned long long)incl);
    base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 63, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 63, 64);
    unsigned long long at = base + incl - mine;
    while (hit) {
        const int bit = __ffsll((long long)hit) - 1;
        hit &= hit - 1ull;
        const int e = bit & 15, ti = bit >> 5, tj = (bit >> 4) & 1;
        const uint32_t a = row0 + (uint32_t)(f.wr * 64 + ti * 32 + (e & 3) + 8 * (e >> 2) + 4 * f.lh);
        const uint32_t b = col0 + (uint32_t)(f.wc * 64 + tj * 32 + f.l31);
        if (at < cap) cand[at] = make_uint2(a, b);
        ++at;
    }
}

// The m residue slots of a row (assign_multi_kernels.h): slot j holds the running maximum, as an ordered int, of the coarse
// value v = acc * (1 / w_b) over the columns c with c % m == j that are there and unmarked; slot j of tile row r lies at
// slots[j * SLOT_STRIDE + r].  This folds one tile's accumulators in (cw0 / cw1: the weights of this lane's two columns,
// cl0 and cl0 + 32 of the tile).  A NaN never enters a slot.
constexpr int SLOT_MAX_M = 16;                             // slots per row
constexpr int SLOT_STRIDE = TILE + 4;                      // ints between a row's slots: the 16 slots start 4 banks apart
__device__ __forceinline__ void tile_slots_max(int* slots, const float* roww, const TileFrag& f, const f32x16 (&acc)[2][2], uint32_t col0,
                                               uint32_t m, float cw0, float cw1) {
    const float ninf = -__uint_as_float(0x7F800000u);
    const int cl0 = f.wc * 64 + f.l31, cl1 = cl0 + 32;
    int* p0 = slots + ((col0 + (uint32_t)cl0) % m) * SLOT_STRIDE + f.wr * 64 + 4 * f.lh;
    int* p1 = slots + ((col0 + (uint32_t)cl1) % m) * SLOT_STRIDE + f.wr * 64 + 4 * f.lh;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ro = ti * 32 + 8 * q;
            const f32x4 wa = *reinterpret_cast<const f32x4*>(roww + f.wr * 64 + 4 * f.lh + ro);
            const i32x4 mo0 = *reinterpret_cast<const i32x4*>(p0 + ro);
            const i32x4 mo1 = *reinterpret_cast<const i32x4*>(p1 + ro);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ob0 = tile_ord(fmaxf(ninf, acc[ti][0][4 * q + j] * cw0));
                const int ob1 = tile_ord(fmaxf(ninf, acc[ti][1][4 * q + j] * cw1));
                if (wa[j] > 0.0f && cw0 > 0.0f && ob0 > mo0[j]) atomicMax(p0 + ro + j, ob0);
                if (wa[j] > 0.0f && cw1 > 0.0f && ob1 > mo1[j]) atomicMax(p1 + ro + j, ob1);
            }
        }
    }
}

}  // namespace mi
