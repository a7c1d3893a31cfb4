// ordered_kernels.h — device code of mi_knn_search_ordered and mi_knn_stamp_histogram: what runs behind the distance scan.
//
// The scan (knn_page_scan_kernel<NCH, 1>, no cursor) has left one 32-bit distance key per entry — a row of the table or an entry
// of the predicate's ascending list — with 0xFFFFFFFF for everything outside the distance bound, deleted rows included.  From
// here on there are integers only.  An entry is SELECTABLE iff its distance key is not 0xFFFFFFFF and it lies past the cursor
// (ordered_host.h: ordered_past).  Its selection key has 96 bits: (okey(stamp) : 64, position : 32).  Lists ascend by row, rows
// ascend with ids, so the key order is the result order (okey, id), and a key is unique per entry: there is one answer.
//
// The k smallest keys are found by the search's most-significant-digit radix select (knn_select_* in knn_kernels.h), widened:
// nine digits — 11, 11, 11, 11, 10, 10 bits of the stamp word, then 11, 11, 10 of the position — one histogram pass per digit
// into 2048 LDS bins flushed with integer atomics; every block of pass p derives the pick of pass p-1 from that pass's complete
// histogram (all reach the same answer), so no workgroup waits for another.  Fewer selectable entries than k (seen in the first
// histogram's total), or a picked bin that holds exactly the wanted rank, decide the state: the later passes return at once.  The
// position passes therefore run only when the k-th stamp is shared by more entries than fit — always in a table whose stamps
// are all the default.  ordered_collect_kernel gathers the keys <= the k-th (at most k), one block sorts them, and
// ordered_finish_kernel maps every slot to id, distance (from the entry's distance key) and stamp.  Atomics add integers: the
// result does not depend on the grid or on the order in which blocks arrive.
#pragma once
#include "../../include/mi355clip.h"
#include "knn_shared.h"
#include "ordered_host.h"

namespace mi {

constexpr int ORD_BINS = 2048, ORD_PASSES = 9, ORD_STAMP_PASSES = 6;
// the words of the select block: ORD_PASSES histograms | the states | the collect counter
struct OrdState { uint64_t hi; uint32_t lo, k_rem; int done, fixed; };
static_assert(sizeof(OrdState) == 24, "layout of the state words");
constexpr size_t ORD_HIST_WORDS = (size_t)ORD_PASSES * ORD_BINS;
constexpr size_t ORD_STATE_WORDS = (size_t)ORD_PASSES * sizeof(OrdState) / sizeof(uint32_t);
constexpr size_t ORD_SEL_WORDS = ORD_HIST_WORDS + ORD_STATE_WORDS + 2;

// digit p: passes 0..5 cut the stamp word, 6..8 the position word
__device__ __forceinline__ int ord_shift(int p) {
    return p == 0 ? 53 : p == 1 ? 42 : p == 2 ? 31 : p == 3 ? 20 : p == 4 ? 10 : p == 5 ? 0 : p == 6 ? 21 : p == 7 ? 10 : 0;
}
__device__ __forceinline__ uint32_t ord_mask(int p) { return (p == 4 || p == 5 || p == 8) ? 0x3FFu : 0x7FFu; }
__device__ __forceinline__ uint32_t ord_digit(int p, uint64_t hi, uint32_t lo) {
    return p < ORD_STAMP_PASSES ? (uint32_t)(hi >> ord_shift(p)) & ord_mask(p) : (lo >> ord_shift(p)) & ord_mask(p);
}
// does (hi, lo) carry the `fixed` digits chosen so far?
__device__ __forceinline__ bool ord_match(const OrdState& st, uint64_t hi, uint32_t lo) {
    const int f = st.fixed;
    if (f == 0) return true;
    if (f < ORD_STAMP_PASSES) return (hi & (~0ull << ord_shift(f - 1))) == st.hi;
    if (hi != st.hi) return false;
    if (f == ORD_STAMP_PASSES) return true;
    return (lo & (~0u << ord_shift(f - 1))) == st.lo;
}

// The state in front of pass n_pass (n_pass == ORD_PASSES: in front of the collect), made by every block of that kernel from
// the complete histogram of pass n_pass - 1; the sel_advance of knn_kernels.h over nine digits.  k_rem = the rank of the wanted
// key inside the prefix group (1-based); done = the group holds exactly k_rem keys, or (fixed == 0) there are fewer selectable
// entries than k: everything that matches the prefix is taken.
__device__ inline OrdState ord_advance(const uint32_t* __restrict__ hist, OrdState* __restrict__ states, int n_pass, uint32_t k) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t s_bin, s_rem, s_cnt;
    OrdState st{0ull, 0u, k, 0, 0};
    if (n_pass == 0) return st;
    if (n_pass >= 2) st = states[n_pass - 2];
    if (st.done) {  // decided earlier: hand the verdict on (the next kernel reads states[n_pass - 1])
        if (threadIdx.x == 0) states[n_pass - 1] = st;
        return st;
    }
    const int p = n_pass - 1;
    const uint32_t* h = hist + p * ORD_BINS;
    uint32_t mine[8], loc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { mine[j] = h[threadIdx.x * 8 + j]; loc += mine[j]; }
    part[threadIdx.x] = loc;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 partials
        const uint32_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t incl = part[threadIdx.x], excl = incl - loc, total = part[255];
    if (total < st.k_rem) {  // only in front of pass 1: fewer selectable entries than k, all are taken
        __syncthreads();
        st.done = 1;
        if (threadIdx.x == 0) states[p] = st;
        return st;
    }
    if (excl < st.k_rem && st.k_rem <= incl) {  // exactly one thread: the wanted rank falls into its 8 bins
        uint32_t acc = excl;
        int j = 0;
        while (j < 7 && acc + mine[j] < st.k_rem) acc += mine[j++];
        s_bin = threadIdx.x * 8 + j; s_rem = st.k_rem - acc; s_cnt = mine[j];
    }
    __syncthreads();
    if (p < ORD_STAMP_PASSES) st.hi |= (uint64_t)s_bin << ord_shift(p);
    else st.lo |= s_bin << ord_shift(p);
    st.k_rem = s_rem;
    st.done = s_cnt == s_rem;  // the whole group is wanted: its lower digits do not matter
    st.fixed = p + 1;
    if (threadIdx.x == 0) states[p] = st;  // every block writes the same words
    __syncthreads();
    return st;
}

// entry e of the n: is it selectable, and its key.  keys32 [n]; list (nullable): entry -> local row; stamps (nullable): per
// local row, a table without the column holds 0 everywhere
struct OrdEntry { bool ok, within; uint64_t hi; };
__device__ __forceinline__ OrdEntry ord_entry(uint64_t e, uint64_t n, const uint32_t* __restrict__ keys32,
                                              const uint32_t* __restrict__ list, const long long* __restrict__ stamps,
                                              const OrderedCursor& cur) {
    OrdEntry r{false, false, 0ull};
    if (e >= n) return r;
    r.within = keys32[e] != 0xFFFFFFFFu;
    if (!r.within) return r;
    const uint64_t row = list ? (uint64_t)list[e] : e;
    r.hi = ordered_okey(stamps ? (int64_t)stamps[row] : (int64_t)0, cur.desc != 0);
    r.ok = ordered_past(cur, r.hi, row);
    return r;
}

// pass p: the histogram of digit p over the selectable entries that carry the prefix chosen so far.  Pass 0 also counts the
// entries within the bound that the cursor leaves behind: ballots, one atomic per wave.  grid: any number of 256-thread blocks
__global__ __launch_bounds__(256) void ordered_hist_kernel(const uint32_t* __restrict__ keys32, uint64_t n,
                                                           const uint32_t* __restrict__ list, const long long* __restrict__ stamps,
                                                           OrderedCursor cur, uint32_t k, int p, uint32_t* __restrict__ hist,
                                                           OrdState* __restrict__ states, unsigned long long* __restrict__ before) {
    __shared__ uint32_t lh[ORD_BINS];
    const OrdState st = ord_advance(hist, states, p, k);
    if (st.done) return;
    for (int j = threadIdx.x; j < ORD_BINS; j += 256) lh[j] = 0;
    __syncthreads();
    uint32_t n_before = 0;
    // whole waves walk the entries: the ballots below need every lane of a wave in the same iteration
    const uint64_t n_round = (n + 63) & ~63ull;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n_round; e += (uint64_t)gridDim.x * 256) {
        const OrdEntry en = ord_entry(e, n, keys32, list, stamps, cur);
        if (p == 0) n_before += (uint32_t)__popcll(__ballot(en.within && !en.ok));
        const bool hit = en.ok && ord_match(st, en.hi, (uint32_t)e);
        const uint32_t bin = ord_digit(p, en.hi, (uint32_t)e);
        // stamps of one corpus crowd into a few leading digits, and a column of few distinct values into a few bins in every
        // pass: a bin shared by lanes of the wave is added once by one lane (up to 8 bins; beyond that the lanes add for
        // themselves)
        unsigned long long left = __ballot(hit);
        for (int round = 0; round < 8 && left != 0ull; ++round) {
            const uint32_t first = __builtin_amdgcn_readfirstlane(__shfl((int)bin, __ffsll((long long)left) - 1, 64));
            const unsigned long long same = __ballot(hit && bin == first) & left;
            if ((threadIdx.x & 63) == 0) atomicAdd(&lh[first], (uint32_t)__popcll(same));
            left &= ~same;
        }
        if ((left >> (threadIdx.x & 63)) & 1ull) atomicAdd(&lh[bin], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < ORD_BINS; j += 256)
        if (lh[j]) atomicAdd(&hist[p * ORD_BINS + j], lh[j]);
    if (p == 0 && (threadIdx.x & 63) == 0 && n_before) atomicAdd(before, (unsigned long long)n_before);
}

// every selectable key <= the k-th smallest goes to out_hi / out_lo (unordered); *count = how many (<= k by construction)
__global__ __launch_bounds__(256) void ordered_collect_kernel(const uint32_t* __restrict__ keys32, uint64_t n,
                                                              const uint32_t* __restrict__ list, const long long* __restrict__ stamps,
                                                              OrderedCursor cur, uint32_t k, const uint32_t* __restrict__ hist,
                                                              OrdState* __restrict__ states, uint64_t* __restrict__ out_hi,
                                                              uint32_t* __restrict__ out_lo, uint32_t* __restrict__ count) {
    const OrdState st = ord_advance(hist, states, ORD_PASSES, k);
    // done: the whole prefix group; otherwise all nine digits are fixed and the prefix IS the k-th key
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
        const OrdEntry en = ord_entry(e, n, keys32, list, stamps, cur);
        if (!en.ok) continue;
        const uint32_t lo = (uint32_t)e;
        bool take;
        if (st.fixed == 0) {
            take = true;
        } else if (st.fixed <= ORD_STAMP_PASSES) {
            const uint64_t t_hi = st.hi | ((1ull << ord_shift(st.fixed - 1)) - 1ull);
            take = en.hi <= t_hi;
        } else {
            const uint32_t t_lo = st.lo | ((1u << ord_shift(st.fixed - 1)) - 1u);
            take = en.hi < st.hi || (en.hi == st.hi && lo <= t_lo);
        }
        if (take) {
            const uint32_t at = atomicAdd(count, 1u);
            if (at < k) { out_hi[at] = en.hi; out_lo[at] = lo; }
        }
    }
}

// one block: the (<= 4096) collected keys ascending by (hi, lo) into out_hi / out_lo [0, min(*count, k))
__global__ __launch_bounds__(1024) void ordered_sort_kernel(const uint64_t* __restrict__ in_hi, const uint32_t* __restrict__ in_lo,
                                                            const uint32_t* __restrict__ count, uint32_t k,
                                                            uint64_t* __restrict__ out_hi, uint32_t* __restrict__ out_lo) {
    __shared__ uint64_t bh[4096];
    __shared__ uint32_t bl[4096];
    const uint32_t n = min(*count, k);
    int np = 64;
    while ((uint32_t)np < k) np <<= 1;  // the power of two that holds k (<= 4096)
    for (int j = threadIdx.x; j < np; j += 1024) {
        bh[j] = (uint32_t)j < n ? in_hi[j] : ~0ull;
        bl[j] = (uint32_t)j < n ? in_lo[j] : ~0u;
    }
    __syncthreads();
    for (int kk = 2; kk <= np; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < np / 2; p += 1024) {
                const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1)), b = a | j;
                const uint64_t xh = bh[a], yh = bh[b];
                const uint32_t xl = bl[a], yl = bl[b];
                const bool up = (a & kk) == 0;
                const bool gt = xh > yh || (xh == yh && xl > yl);
                if (gt == up && (xh != yh || xl != yl)) { bh[a] = yh; bh[b] = xh; bl[a] = yl; bl[b] = xl; }
            }
            __syncthreads();
        }
    for (uint32_t j = threadIdx.x; j < n; j += 1024) { out_hi[j] = bh[j]; out_lo[j] = bl[j]; }
}

// The sorted keys -> idx / dist / stamps; one thread per result slot, padding behind the min(*count, k) hits.  The distance
// comes from the entry's distance key, as knn_page_finish_kernel's does: a key maps back to one float.
__global__ void ordered_finish_kernel(const uint64_t* __restrict__ s_hi, const uint32_t* __restrict__ s_lo,
                                      const uint32_t* __restrict__ count, uint32_t k, const uint32_t* __restrict__ keys32,
                                      const uint32_t* __restrict__ list, int desc, IdMap map, uint64_t* __restrict__ idx,
                                      float* __restrict__ dist, long long* __restrict__ stamps) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const bool hit = j < min(*count, k);
    uint64_t id = MI_KNN_NO_ID;
    float d = __uint_as_float(0x7F800000u);
    long long st = 0;
    if (hit) {
        const uint32_t pos = s_lo[j];
        id = id_of_local(map, list ? list[pos] : pos);
        d = u32_to_dist(keys32[pos]);
        st = (long long)ordered_stamp_of(s_hi[j], desc != 0);
    }
    idx[j] = id;
    dist[j] = d;
    stamps[j] = st;
}

// The timeline facet: hist[b] += the entries within the bound whose stamp has exactly b edges <= it.  The edges (<= 4096,
// strictly ascending) and the block's counts live in LDS; a lane binary-searches its entry's stamp; LDS integer atomics count,
// one 64-bit global atomic per non-zero bin and block flushes.  grid: any number of 256-thread blocks
__global__ __launch_bounds__(256) void ordered_stamp_hist_kernel(const uint32_t* __restrict__ keys32, uint64_t n,
                                                                 const uint32_t* __restrict__ list,
                                                                 const long long* __restrict__ stamps,
                                                                 const long long* __restrict__ edges, uint32_t n_edges,
                                                                 unsigned long long* __restrict__ hist) {
    __shared__ long long s_edges[ORDERED_EDGES_MAX];
    __shared__ uint32_t s_cnt[ORDERED_EDGES_MAX + 1];
    for (uint32_t j = threadIdx.x; j < n_edges; j += 256) s_edges[j] = edges[j];
    for (uint32_t j = threadIdx.x; j <= n_edges; j += 256) s_cnt[j] = 0;
    __syncthreads();
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
        if (keys32[e] == 0xFFFFFFFFu) continue;
        const uint64_t row = list ? (uint64_t)list[e] : e;
        const long long st = stamps ? stamps[row] : 0ll;
        uint32_t lo = 0, hi = n_edges;   // the first edge above the stamp = the number of edges <= it
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_edges[mid] <= st) lo = mid + 1;
            else hi = mid;
        }
        atomicAdd(&s_cnt[lo], 1u);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j <= n_edges; j += 256)
        if (s_cnt[j]) atomicAdd(&hist[j], (unsigned long long)s_cnt[j]);
}

}  // namespace mi
