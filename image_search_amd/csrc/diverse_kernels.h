// diverse_kernels.h — device code of mi_knn_search_diverse: the k best DISTINCT results of a search, the look-alikes of each
// counted behind it.  The search's own list of `pool` entries stays on the device; everything below works on that list.
//
// diverse_pool_kernel.  Drops the padding and the NaN entries (what is left keeps the search's order: rank r = 0 .. P-1),
// turns ids into local rows, and copies the P fp32 rows into a contiguous [P][dim] buffer — at the POSITION the row has
// among the pool's local rows in ascending order.  Why that order: the pair distance of the contract is the one
// mi_knn_search(q = row lo) reports for row hi, lo < hi the ids; join_tiles_kernel emits pairs (a, b) with a < b and the
// rescore takes a as the query.  With positions in id order a position pair a < b IS an id pair lo < hi, and the distance
// has the bits mi_knn_near_pairs would report.  (1 - q.x / (|q| |x|) is symmetric in exact arithmetic only: the query's norm
// is summed once and the streamed row's with the dot product, the two roles round differently.)  At most 4096 entries: a
// counting rank (position = number of pool rows with a smaller local row) serves; every workgroup redoes the compaction
// of the whole list (4096 loads and a scan) and ranks and gathers DIV_PER_BLOCK entries of its own.
//
// Stage 1 is join_tiles_kernel over the bf16 mirror of the gathered copy (mirror_rows), stage 2 diverse_rescore_kernel:
// the pair-distance block of join_rescore_kernel (join_kernels.h), and instead of compacting (a, b, dist) it sets bit
// (max rank, min rank) of a P x P conflict matrix (rows of DIV_WORDS 64-bit words) with an atomicOr: order-free, so neither
// the candidates' arrival order nor the way an overflowing strip was cut shows in the result.  The bound eps2 makes the
// stage exact as for the join: a pair with exact distance <= min_gap has coarse distance <= min_gap + eps2 and is a candidate.
//
// diverse_select_kernel: the greedy walk, one workgroup.  The kept set is 4096 bits, one 64-bit word per lane of wave 0.
// Step r: row r of the matrix AND the kept set; a ballot finds the first lane with a bit left, v_readlane fetches that
// word, its lowest bit is F, the kept entry of smallest rank that conflicts.  No F and fewer than k kept: r is kept.  The
// matrix comes through LDS in images of DIV_CHUNK rows, the next image loaded by all four waves while wave 0 walks the
// current one, and inside an image row r + 1 is read before row r is decided (neither load depends on the walk's state).
// The walk records for each rank only WHICH rank it went behind; slots, hidden counts and the outputs are filled in by the
// whole workgroup afterwards, so the serial part holds no dependent LDS read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "knn_shared.h"

namespace mi {

constexpr uint32_t DIV_MAX_POOL = 4096;
constexpr int DIV_WORDS = DIV_MAX_POOL / 64;   // 64-bit words of one row of the conflict matrix
constexpr int DIV_CHUNK = 32;                  // matrix rows per LDS image (16 KiB)
constexpr int DIV_PER_BLOCK = 16;              // pool entries a workgroup of diverse_pool_kernel ranks and gathers
constexpr uint32_t DIV_NONE = 0xFFFFu;         // "behind nothing and not kept" in the walk's 16-bit record

// grid: ceil(pool / DIV_PER_BLOCK) workgroups.  s_idx / s_dist: the search's list [pool].  An entry is in the pool when its
// id is a row of the table (base <= id < base + n_rows: never false for what the search wrote, and it keeps the gather
// inside the table) and its distance is not NaN.  p_idx / p_dist: the pool in rank order; rank_of_pos[position] = rank;
// copy: [P][dim]; *n_pool = P.
__global__ __launch_bounds__(256) void diverse_pool_kernel(const float* __restrict__ table, uint32_t dim, uint64_t n_rows, uint64_t base,
                                                           const uint64_t* __restrict__ s_idx, const float* __restrict__ s_dist,
                                                           uint32_t pool, uint64_t* __restrict__ p_idx, float* __restrict__ p_dist,
                                                           uint32_t* __restrict__ rank_of_pos, float* __restrict__ copy,
                                                           uint32_t* __restrict__ n_pool) {
    __shared__ uint32_t local_of[DIV_MAX_POOL];   // rank -> local row
    __shared__ uint16_t orig_of[DIV_MAX_POOL];    // rank -> index in the search's list
    __shared__ uint32_t wave_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    constexpr int PER = DIV_MAX_POOL / 256;       // consecutive entries of the list per thread

    uint32_t valid = 0, mine[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t i = (uint32_t)tid * PER + j;
        mine[j] = 0;
        if (i < pool) {
            const uint64_t id = s_idx[i];
            const float d = s_dist[i];
            if (id != MI_KNN_NO_ID && d == d && id >= base && id - base < n_rows) {
                valid |= 1u << j;
                mine[j] = (uint32_t)(id - base);
            }
        }
    }
    const uint32_t cnt = (uint32_t)__popc(valid);
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wave_sum[wib] = incl;
    __syncthreads();
    uint32_t before = incl - cnt, P = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wib) before += wave_sum[w];
        P += wave_sum[w];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (valid & (1u << j)) {
            local_of[before] = mine[j];
            orig_of[before] = (uint16_t)((uint32_t)tid * PER + j);
            ++before;
        }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) *n_pool = P;

    // a 16-lane group per entry: its position = how many pool rows lie below its local row
    const uint32_t r = blockIdx.x * DIV_PER_BLOCK + (uint32_t)(tid >> 4);
    const int sub = tid & 15;
    const bool there = r < P;
    const uint32_t me = there ? local_of[r] : 0u;
    uint32_t below = 0;
    for (uint32_t j = (uint32_t)sub; j < P; j += 16) below += local_of[j] < me ? 1u : 0u;
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) below += __shfl_xor(below, d, 16);
    if (!there) return;
    const uint32_t pos = below;   // < P: the ids of a search's list are distinct
    if (sub == 0) {
        const uint32_t o = orig_of[r];
        p_idx[r] = s_idx[o];
        p_dist[r] = s_dist[o];
        rank_of_pos[pos] = r;
    }
    const f32x4* src = reinterpret_cast<const f32x4*>(table + (uint64_t)me * dim);
    f32x4* dst = reinterpret_cast<f32x4*>(copy + (uint64_t)pos * dim);
    for (uint32_t c = (uint32_t)sub; c < dim / 4; c += 16) dst[c] = src[c];
}

// stage 2: C candidate pairs of positions (a < b) in the gathered copy -> bit (max rank, min rank) of `conflict` for every
// pair with exact distance <= min_gap (never a NaN); *n_conflicts counts them.  The distance is join_rescore_kernel's, line
// for line: position a is the query, position b is streamed.
template <int NCH>
__global__ __launch_bounds__(256) void diverse_rescore_kernel(const float* __restrict__ table, const uint2* __restrict__ cand, uint32_t C,
                                                              float min_gap, const uint32_t* __restrict__ rank_of_pos,
                                                              unsigned long long* __restrict__ conflict,
                                                              uint32_t* __restrict__ n_conflicts) {
    constexpr int DIM = NCH * 64;
    const int lane = threadIdx.x & 63, i = lane & 15;
    const uint32_t group = (blockIdx.x * 256 + threadIdx.x) >> 4, n_groups = (gridDim.x * 256) >> 4;
    // (whole waves stay in the loop: row16_sum and the ballot are cross-lane operations)
    for (uint32_t c0 = group; c0 < ((C + n_groups - 1) / n_groups) * n_groups; c0 += n_groups) {
        const bool live = c0 < C;
        const uint2 pr = cand[live ? c0 : 0];
        const f32x4* pa = reinterpret_cast<const f32x4*>(table + (uint64_t)pr.x * DIM) + i;
        const f32x4* pb = reinterpret_cast<const f32x4*>(table + (uint64_t)pr.y * DIM) + i;
        // (pair_dist of pair_kernels.h, written out: as a call it compiles to another register allocation here at NCH >= 8)
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
        for (int t = 0; t < NCH; ++t) a.step(qf[t], __builtin_nontemporal_load(pb + 16 * t));
        const float d = a.dot(), s = a.sumsq();
        const float dist = 1.0f - d / (sq * sqrtf(s));
        const bool keep = live && i == 0 && dist <= min_gap;
        const unsigned long long m = __ballot(keep);
        if (m == 0ull) continue;
        if (keep) {
            const uint32_t ra = rank_of_pos[pr.x], rb = rank_of_pos[pr.y];
            const uint32_t hi = max(ra, rb), lo = min(ra, rb);
            atomicOr(conflict + (size_t)hi * DIV_WORDS + (lo >> 6), 1ull << (lo & 63));
        }
        if (lane == 0) atomicAdd(n_conflicts, (uint32_t)__popcll(m));
    }
}

// The walk.  One workgroup of 256.  conflict: ceil(P / DIV_CHUNK) * DIV_CHUNK rows of DIV_WORDS words (whole images are
// loaded).  idx / dist / hidden: [k]; rep: [pool]; state: {n_kept, pool entries hidden}.
__global__ __launch_bounds__(256) void diverse_select_kernel(const unsigned long long* __restrict__ conflict, const uint32_t* __restrict__ n_pool,
                                                             const uint64_t* __restrict__ p_idx, const float* __restrict__ p_dist, uint32_t k,
                                                             uint32_t pool, uint64_t* __restrict__ idx, float* __restrict__ dist,
                                                             uint32_t* __restrict__ hidden, uint32_t* __restrict__ rep,
                                                             uint32_t* __restrict__ state) {
    constexpr int IMG_BYTES = DIV_CHUNK * DIV_WORDS * 8;
    __shared__ __attribute__((aligned(16))) unsigned char img[2 * IMG_BYTES];
    __shared__ uint16_t first_of[DIV_MAX_POOL];   // rank -> the rank it went behind (its own when kept, DIV_NONE when left over)
    __shared__ uint16_t slot_of[DIV_MAX_POOL];    // kept rank -> slot
    __shared__ uint16_t rank_of[DIV_MAX_POOL];    // slot -> rank
    __shared__ uint32_t sh_kept, sh_hidden;
    const int tid = threadIdx.x, lane = tid & 63;
    const bool walker = __builtin_amdgcn_readfirstlane(tid >> 6) == 0;
    const uint32_t P = min(*n_pool, min(pool, DIV_MAX_POOL));
    const uint32_t n_chunks = (P + DIV_CHUNK - 1) / DIV_CHUNK;
    const unsigned char* g = reinterpret_cast<const unsigned char*>(conflict);

    u32x4 st[4];
    auto fetch = [&](uint32_t c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) st[j] = *reinterpret_cast<const u32x4*>(g + (size_t)c * IMG_BYTES + (size_t)(tid + 256 * j) * 16);
    };
    auto stash = [&](uint32_t buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x4*>(img + buf * IMG_BYTES + (tid + 256 * j) * 16) = st[j];
    };
    if (tid == 0) { sh_kept = 0; sh_hidden = 0; }
    if (n_chunks) { fetch(0); stash(0); }
    __syncthreads();

    unsigned long long kept = 0ull;   // wave 0: lane w holds ranks 64 w .. 64 w + 63
    uint32_t n_kept = 0;
#pragma unroll 1
    for (uint32_t c = 0; c < n_chunks; ++c) {
        if (c + 1 < n_chunks) fetch(c + 1);
        if (walker) {
            const unsigned long long* rows = reinterpret_cast<const unsigned long long*>(img + (c & 1) * IMG_BYTES);
            const uint32_t nr = min((uint32_t)DIV_CHUNK, P - c * DIV_CHUNK);
            unsigned long long next = rows[lane];
#pragma unroll 1
            for (uint32_t rr = 0; rr < nr; ++rr) {
                const unsigned long long x = next & kept;
                if (rr + 1 < nr) next = rows[(rr + 1) * DIV_WORDS + lane];
                const uint32_t r = c * DIV_CHUNK + rr;
                const unsigned long long m = __ballot(x != 0ull);
                uint32_t f;
                if (m != 0ull) {
                    const int w = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
                    const uint32_t xl = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, w);
                    const uint32_t xh = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), w);
                    f = (uint32_t)w * 64u + (xl ? (uint32_t)__builtin_ctz(xl) : 32u + (uint32_t)__builtin_ctz(xh));
                } else if (n_kept < k) {
                    f = r;
                    if ((uint32_t)lane == (r >> 6)) kept |= 1ull << (r & 63);
                    if (lane == 0) { slot_of[r] = (uint16_t)n_kept; rank_of[n_kept] = (uint16_t)r; }
                    ++n_kept;
                } else {
                    f = DIV_NONE;
                }
                if (lane == 0) first_of[r] = (uint16_t)f;
            }
        }
        // the other image's last reader (the walk over chunk c - 1) passed the barrier that ended the previous step
        if (c + 1 < n_chunks) stash((c + 1) & 1);
        __syncthreads();
    }
    if (walker && lane == 0) sh_kept = n_kept;
    uint32_t* hid = reinterpret_cast<uint32_t*>(img);   // the images are done with: [k] hidden counts
    for (uint32_t j = (uint32_t)tid; j < k; j += 256) hid[j] = 0;
    __syncthreads();
    n_kept = sh_kept;

    for (uint32_t r0 = 0; r0 < pool; r0 += 256) {
        const uint32_t r = r0 + (uint32_t)tid;
        uint32_t v = MI_KNN_NO_LABEL;
        bool behind = false;
        if (r < P) {
            const uint32_t f = first_of[r];
            if (f != DIV_NONE) {
                v = slot_of[f];
                behind = f != r;
                if (behind) atomicAdd(&hid[v], 1u);
            }
        }
        if (r < pool) rep[r] = v;
        const unsigned long long bm = __ballot(behind);
        if (lane == 0 && bm != 0ull) atomicAdd(&sh_hidden, (uint32_t)__popcll(bm));
    }
    __syncthreads();
    for (uint32_t j = (uint32_t)tid; j < k; j += 256) {
        if (j < n_kept) {
            const uint32_t r = rank_of[j];
            idx[j] = p_idx[r];
            dist[j] = p_dist[r];
            hidden[j] = hid[j];
        } else {
            idx[j] = MI_KNN_NO_ID;
            dist[j] = __uint_as_float(0x7F800000u);
            hidden[j] = 0;
        }
    }
    if (tid == 0) { state[0] = n_kept; state[1] = sh_hidden; }
}

}  // namespace mi
