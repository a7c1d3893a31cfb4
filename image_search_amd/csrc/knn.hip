// knn.hip — host side of Seam B behind the C ABI (include/mi355clip.h).
// One mi_knn = one row-shard of the reference's `image.embedding` column
// (server/src/search.rs:13-18) resident in HBM on one GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unistd.h>

#include <iterator>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "common.h"
#include "handles.h"
#include "knn_kernels.h"
#include "where_host.h"

using namespace mi;

namespace {

constexpr int MAX_BATCH_Q = 8;

// the handle's own stream, created on first use (an idle stream still takes one of the four
// hardware queues HIP multiplexes streams onto)
hipStream_t own_stream(mi_knn* t) {
    return t->stream.get(hipStreamNonBlocking);
}

// ---- deleted rows (handles.h: dead, d_tomb, d_dead) -------------------------------------------------------------
// the bitmap the kernels consult, or nullptr: a table without deletions runs the kernels it ran before they existed
const uint64_t* tomb_of(const mi_knn* t) { return t->dead.empty() ? nullptr : t->d_tomb; }

// Arrays that keep one element (or bit) per row of capacity cover n elements: the elements they gain hold the byte `fill`, the
// old contents are carried over.  Nothing in flight may use the old arrays.  Every new array is allocated before an old one
// is replaced, so a failed allocation (MI_ERR_OOM) leaves the handle as it was.
template <class... T>
void fit(mi_knn* t, size_t n, int fill, DevArray<T>&... a) {
    if (((a.p && a.cap >= n) && ...)) return;
    t->writes.sync();
    t->reads.sync();
    std::tuple<DevArray<T>...> grown;
    std::apply([&](auto&... g) {
        (g.alloc(n), ...);
        // the fills and the carry-over copies on the handle's own stream, and waited for: that stream does not order itself
        // behind the null stream, and what is enqueued on it next (an upload, the bits of a deletion) must not be overtaken
        hipStream_t s = own_stream(t);
        (HIP_CHECK(hipMemsetAsync(g.p, fill, n * sizeof(*g.p), s)), ...);
        ((a.p ? HIP_CHECK(hipMemcpyAsync(g.p, a.p, a.cap * sizeof(*g.p), hipMemcpyDeviceToDevice, s)) : (void)0), ...);
        HIP_CHECK(hipStreamSynchronize(s));
        (a.swap(g), ...);
    }, grown);
}
// the deletion bitmap: one bit per row of capacity, the words it gains are zero
void tomb_fit(mi_knn* t) { fit(t, std::max<size_t>((size_t)((t->cap + 63) / 64), 1), 0, t->d_tomb); }

// `rows` (sorted, none deleted yet) join the deleted rows: device list and bitmap on `s`, then the host list
void tomb_add(mi_knn* t, const std::vector<uint32_t>& rows, hipStream_t s) {
    if (rows.empty()) return;
    tomb_fit(t);
    const size_t have = t->dead.size();
    // (grown geometrically: a caller that deletes one row per call must not copy the whole list each time)
    const size_t want = have + rows.size();
    t->d_dead.reserve_keep(t->reads, want > t->d_dead.cap ? std::max(want, 2 * t->d_dead.cap) : want, have);
    HIP_CHECK(hipMemcpyAsync(t->d_dead + have, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const uint32_t n = (uint32_t)rows.size();
    hipLaunchKernelGGL(knn_tomb_set_kernel, dim3(std::max(1u, std::min<uint32_t>((n + 255) / 256, (uint32_t)t->n_cu * 4))), dim3(256), 0, s,
                       t->d_dead + have, n, (unsigned long long*)t->d_tomb.p);
    HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> merged(have + rows.size());
    std::merge(t->dead.begin(), t->dead.end(), rows.begin(), rows.end(), merged.begin());
    t->dead.swap(merged);
}

// the device side rebuilt from the host list (after a truncation or a load); waits for the handle's work in flight
void tomb_rebuild(mi_knn* t) {
    if (!t->d_tomb && t->dead.empty()) return;
    tomb_fit(t);
    t->writes.sync();
    t->reads.sync();
    HIP_CHECK(hipMemsetAsync(t->d_tomb, 0, t->d_tomb.cap * sizeof(uint64_t), own_stream(t)));   // (the stream the bits are set on)
    std::vector<uint32_t> rows;
    rows.swap(t->dead);
    tomb_add(t, rows, own_stream(t));
    HIP_CHECK(hipStreamSynchronize(t->stream));
}

void grow(mi_knn* t, uint64_t want_rows) {
    if (want_rows <= t->cap) return;
    uint64_t ncap = std::max<uint64_t>(want_rows, t->cap + t->cap / 2);
    ncap = (ncap + 63) & ~63ull;
    if (ncap > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "a shard holds at most 2^32-1 rows (asked %llu)",
                                    (unsigned long long)want_rows);
    // the table moves: everything enqueued against the old allocation must have finished
    t->writes.sync();
    t->reads.sync();
    {
        DevArray<float> nt;
        nt.alloc(ncap * t->dim);
        if (t->rows) {
            HIP_CHECK(hipMemcpyAsync(nt, t->table, t->rows * t->dim * sizeof(float), hipMemcpyDeviceToDevice, own_stream(t)));
            HIP_CHECK(hipStreamSynchronize(t->stream));
        }
        t->table.swap(nt);   // the old rows are freed here, before the columns grow
    }
    t->cap = ncap;
    if (t->d_tomb) tomb_fit(t);  // the deletion bitmap keeps one bit per row of capacity
    if (t->d_groups) knn_groups_fit(t);  // the group column one id
    if (t->d_tags) knn_attrs_fit(t);     // the attribute columns one word each
}

template <class K>
void allow_lds(K kernel, size_t bytes) {
    if (bytes > 48 * 1024)
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// gy > 1: a group of queries in one launch (grid.y = query, knn_kernels.h QGroup)
template <class Top>
void launch_scan(mi_knn* t, const float* d_q, uint32_t k, const uint64_t* lo, uint64_t* cand, uint32_t blocks,
                 hipStream_t s, const uint32_t* run_if = nullptr, uint32_t gy = 1, QGroup qg = QGroup{}) {
    const size_t lds = (size_t)4 * Top::LDS_KEYS * sizeof(uint64_t);
    const uint64_t* tomb = tomb_of(t);
    switch (t->dim / 64) {
#define MI_CASE(NCH)                                                                                   \
    case NCH:                                                                                          \
        if (tomb) {                                                                                    \
            allow_lds(knn_scan_kernel<NCH, Top, 0, true>, lds);                                        \
            hipLaunchKernelGGL((knn_scan_kernel<NCH, Top, 0, true>), dim3(blocks, gy), dim3(256), lds, s, \
                               t->table, t->rows, d_q, k, lo, cand, (uint32_t*)nullptr, run_if, qg, tomb); \
            break;                                                                                     \
        }                                                                                              \
        allow_lds(knn_scan_kernel<NCH, Top>, lds);                                                     \
        hipLaunchKernelGGL((knn_scan_kernel<NCH, Top>), dim3(blocks, gy), dim3(256), lds, s, t->table, \
                           t->rows, d_q, k, lo, cand, (uint32_t*)nullptr, run_if, qg);                 \
        break;
        MI_CASE(1) MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
        default: fail(MI_ERR_UNSUPPORTED, "dim %u: built for dim/64 in {1,2,4,8,12,16}", t->dim);
    }
    HIP_CHECK(hipGetLastError());
}

template <class Top>
void launch_merge(const uint64_t* in, uint32_t n_lists, uint32_t k, uint32_t lpb, uint64_t* out, uint32_t nq,
                  size_t in_stride, size_t out_stride, hipStream_t s, const uint32_t* run_if = nullptr, uint32_t run_stride = 0) {
    const size_t lds = (size_t)4 * Top::LDS_KEYS * sizeof(uint64_t);
    allow_lds(knn_merge_kernel<Top>, lds + 4096);
    const uint32_t blocks = (n_lists + lpb - 1) / lpb;
    hipLaunchKernelGGL((knn_merge_kernel<Top>), dim3(blocks, nq), dim3(256), lds, s, in, n_lists, k, lpb, out,
                       in_stride, out_stride, run_if, run_stride);
    HIP_CHECK(hipGetLastError());
}

template <class Top>
void reduce_wave_lists(mi_knn* t, uint32_t lists, uint32_t kp, uint64_t* keys_out, hipStream_t s, const uint32_t* run_if,
                       uint32_t gy, const QGroup& qg);

// One pass: the kp <= 1024 smallest keys (> *lo if lo) of the shard, ascending, into keys_out[0..kp).
// gy > 1 (register lists only): the same pass for a group of gy queries (contiguous at d_q) in the same launches, query y
// gated by run_if[y * qg.flags], its keys to keys_out + y * qg.out
template <class Top>
void one_pass(mi_knn* t, const float* d_q, uint32_t kp, const uint64_t* lo, uint64_t* keys_out, hipStream_t s,
              const uint32_t* run_if = nullptr, uint32_t gy = 1, QGroup qg = QGroup{}) {
    const uint32_t bpc = Top::LDS_KEYS == 0 ? 4 : (Top::KP <= 256 ? 4 : 2);
    const uint64_t n_tiles = (t->rows + 63) / 64;
    uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * bpc, (n_tiles + 3) / 4);
    blocks = std::max(blocks, 1u);
    const uint32_t lists = blocks * 4;
    t->d_cand.reserve(t->reads, (size_t)lists * kp * gy);
    qg.lists = (uint64_t)lists * kp;
    launch_scan<Top>(t, d_q, kp, lo, t->d_cand, blocks, s, run_if, gy, qg);
    reduce_wave_lists<Top>(t, lists, kp, keys_out, s, run_if, gy, qg);
}

// the per-wave lists in t->d_cand (lists x kp keys per query) -> the kp smallest keys, ascending, into keys_out
template <class Top>
void reduce_wave_lists(mi_knn* t, uint32_t lists, uint32_t kp, uint64_t* keys_out, hipStream_t s, const uint32_t* run_if,
                       uint32_t gy, const QGroup& qg) {
    if constexpr (Top::LDS_KEYS != 0) {
        // k > 64: block-cooperative tree, 16 lists per block per level, ping-pong between d_tmp halves
        constexpr uint32_t LPB = 16;
        t->d_tmp.reserve(t->reads, (size_t)2 * ((lists + LPB - 1) / LPB) * kp);
        const uint64_t* in = t->d_cand;
        uint32_t n = lists, lvl = 0;
        while (true) {
            const uint32_t nb = (n + LPB - 1) / LPB;
            uint64_t* out = nb == 1 ? keys_out : t->d_tmp + (size_t)(lvl & 1) * ((lists + LPB - 1) / LPB) * kp;
            hipLaunchKernelGGL((knn_merge_block_kernel<Top::KP>), dim3(nb), dim3(256), 0, s, in, n, kp, LPB, out);
            HIP_CHECK(hipGetLastError());
            if (nb == 1) break;
            in = out; n = nb; ++lvl;
        }
        return;
    }
    // tree: <= 64 lists per block, then one block
    if (lists <= 64) {
        launch_merge<Top>(t->d_cand, lists, kp, lists, keys_out, gy, qg.lists, qg.out, s, run_if, qg.flags);
    } else {
        const uint32_t lpb = 32, mid = (lists + lpb - 1) / lpb;
        t->d_tmp.reserve(t->reads, (size_t)mid * kp * gy);
        launch_merge<Top>(t->d_cand, lists, kp, lpb, t->d_tmp, gy, qg.lists, (size_t)mid * kp, s, run_if, qg.flags);
        launch_merge<Top>(t->d_tmp, mid, kp, mid, keys_out, gy, (size_t)mid * kp, qg.out, s, run_if, qg.flags);
    }
}

// Two-stage exact search (knn_kernels.h "bf16 mirror as prefilter"): k <= 4096 (the single pass behind it must be one of
// the two gated forms: register lists, or the radix select), dim a multiple of 128, enough rows for the saved bytes to
// outweigh a dozen short launches.  Leaves the answer's keys in d_pref_keys and *fallback == 0, or
// *fallback == 1: the caller enqueues the single pass behind it, gated by that word.
constexpr uint64_t PREF_MIN_ROWS = 1u << 18;
bool prefilter_applies(const mi_knn* t, uint32_t k) {
    const uint32_t width = t->prefilter == 2 ? 256u : 128u;  // whole 256-byte chunks per mirror row
    return t->prefilter && (k <= 64 || (k <= 4096 && t->select_path)) && t->dim % width == 0 && t->rows >= PREF_MIN_ROWS;
}
// sample_shift > 0 (matrix-pipe form only): every 2^shift-th 16-row tile's keys also go, compactly, to t->d_skeys [nq][sample_stride]
template <int NCH>
void launch_coarse8_batched(mi_knn* t, const uint8_t* m8, const float* d_q, float e0, uint32_t nq, uint32_t blocks, hipStream_t s,
                            int sample_shift = 0, uint64_t sample_stride = 0) {
    if constexpr (NCH == 12) {  // built for dim 768, the width of the reference's table (server/src/clip.rs:140-143)
        if (t->batch_stage1_mfma) {
            // the group's stage 1 on the matrix pipe: exact int8 dot products against the query cut into three 7-bit digits
            hipLaunchKernelGGL(knn_query_digits_kernel, dim3(nq), dim3(256), 0, s, d_q, t->d_g8, (int)t->dim, t->d_digits, t->d_qs, t->d_rho8);
            constexpr int LDS = c8m_lds_bytes(NCH * 64);
            const uint64_t n_tiles = (t->rows + 15) / 16;
            const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)t->n_cu, (n_tiles + 3) / 4));   // 153 KB of LDS: one workgroup per CU
#define MI_C8M(NBLK, QPB)                                                                                                         \
    {                                                                                                                             \
        allow_lds(knn_scan_coarse8_mfma_kernel<NCH, NBLK, QPB>, LDS);                                                             \
        hipLaunchKernelGGL((knn_scan_coarse8_mfma_kernel<NCH, NBLK, QPB>), dim3(grid), dim3(256), LDS, s, m8, t->d_xx, t->d_scale8, \
                           t->d_cfac8, t->rows, t->d_digits, t->d_qs, (int)nq, e0, t->d_keys32, (uint64_t)t->cap,                 \
                           sample_shift ? t->d_skeys : (uint32_t*)nullptr, sample_shift, sample_stride);                          \
    }
            if (nq <= 5) MI_C8M(1, 5)
            else if (nq <= 10) MI_C8M(2, 5)
            else if (nq <= 15) MI_C8M(3, 5)
            else MI_C8M(4, 4)
#undef MI_C8M
            HIP_CHECK(hipGetLastError());
            return;
        }
        if (nq == 8)
            hipLaunchKernelGGL((knn_scan_coarse8_batched_kernel<NCH, 8>), dim3(blocks), dim3(256), 0, s, m8, t->d_xx, t->d_scale8, t->d_cfac8,
                               t->d_g8, t->rows, d_q, e0, t->d_keys32, (uint64_t)t->cap, t->d_rho8);
        else if (nq == 2)
            hipLaunchKernelGGL((knn_scan_coarse8_batched_kernel<NCH, 2>), dim3(blocks), dim3(256), 0, s, m8, t->d_xx, t->d_scale8, t->d_cfac8,
                               t->d_g8, t->rows, d_q, e0, t->d_keys32, (uint64_t)t->cap, t->d_rho8);
        else
            hipLaunchKernelGGL((knn_scan_coarse8_batched_kernel<NCH, 4>), dim3(blocks), dim3(256), 0, s, m8, t->d_xx, t->d_scale8, t->d_cfac8,
                               t->d_g8, t->rows, d_q, e0, t->d_keys32, (uint64_t)t->cap, t->d_rho8);
    } else {
        fail(MI_ERR_UNSUPPORTED, "the batched two-stage search is built for dim 768");
    }
}
// the strides of a group of gy queries on the shard's workspaces (every per-query buffer holds gy copies back to back)
constexpr uint32_t SEL_WORDS = 6 * SEL_BINS + 64;
constexpr uint32_t KNN_GROUP_MAX = 16;   // queries that share one pass over the byte mirror (matrix-pipe stage 1; the vector-ALU form: 8)
// how many of `left` >= 2 queries the next group takes: any count up to 16 on the matrix pipe, 8 / 4 / 2 on the vector ALU
uint32_t group_size(const mi_knn* t, uint32_t left) {
    if (t->batch_stage1_mfma) return std::min(left, KNN_GROUP_MAX);
    return left >= 8 ? 8 : left >= 4 ? 4 : 2;
}
QGroup group_of(const mi_knn* t, uint32_t gy) {
    QGroup g;
    if (gy <= 1) return g;
    g.q = t->dim; g.keys = t->cap; g.sel = SEL_WORDS; g.flags = 4; g.rows = (uint64_t)2 * PREF_CAP; g.coll = 4096; g.out = 4096; g.rho = 1;
    return g;
}
// nq_batch = 2 .. KNN_GROUP_MAX (16) (byte mirror, dim 768): a GROUP of queries, contiguous at d_q: one pass over the mirror writes the
// stage-1 keys of all of them, and every later kernel of the search — the selects, the collect, stage 2, the select over the
// candidates, the sort — runs ONCE for the group with the query as grid.y on per-query copies of the workspaces (QGroup).
// Returns the fallback word of query 0 (query y: + 4 y).
uint32_t* prefilter_pass(mi_knn* t, const float* d_q, uint32_t k, hipStream_t s, uint32_t nq_batch = 0) {
    const uint32_t gy = std::max(1u, nq_batch);
    const QGroup qg = group_of(t, gy);
    t->d_keys32.reserve(t->reads, (size_t)t->cap * gy);
    t->d_sel.reserve(t->reads, (size_t)SEL_WORDS * gy);
    t->d_cand.reserve(t->reads, (size_t)4096 * gy);
    t->d_pref_rows.reserve(t->reads, (size_t)2 * PREF_CAP * gy);  // rows, then their exact keys
    t->d_pref_keys.reserve(t->reads, (size_t)4096 * gy);
    t->d_pref_flag.reserve(t->reads, (size_t)4 * gy);
    const bool bytes = t->prefilter == 2;
    // The threshold from a SAMPLE of the keys (byte mirror, k <= 64): stage 1 also writes the keys of every 8th tile compactly,
    // the three histogram passes read that eighth, and the collect pass filters ALL keys against the sample's k-th smallest
    // upper bound — which is >= the k-th smallest over all rows, hence a valid (looser) threshold: a few times more candidates
    // for stage 2 (hundreds instead of tens at k = 10), three quarters of the select's traffic gone.  Tiles of 64 rows for one
    // query, of 16 rows for a group on the matrix pipe; the old vector-ALU group kernel does not sample.
    const uint32_t tile_rows = (nq_batch && t->batch_stage1_mfma) ? 16 : 64;
    const uint64_t n_tiles_s = (t->rows + tile_rows - 1) / tile_rows;
    // (groups only by default: for ONE query the 45 us of histogram reads it saves go into the larger stage 2 — measured equal at
    // k = 10, 2 % slower at k = 64; "prefilter_sample" = 2 samples for single queries too)
    int sample_shift = (bytes && t->pref_sample && k <= 64 && ((nq_batch >= 2 && t->batch_stage1_mfma) || (nq_batch == 0 && t->pref_sample >= 2))) ? 3 : 0;
    uint64_t n_sample = ((n_tiles_s + (1u << sample_shift) - 1) >> sample_shift) * tile_rows;
    if (sample_shift && (t->rows >> sample_shift) < std::max<uint64_t>(4096, 64ull * k)) { sample_shift = 0; n_sample = 0; }   // too small a table: the sample would be no guide
    // sized by the table's CAPACITY, not its rows: a table that grows by a chunk per step (the pipeline) must not reallocate
    // the sample — and wait for the searches in flight — every other query
    const uint64_t sample_stride = sample_shift ? ((((t->cap + tile_rows - 1) / tile_rows + (1u << sample_shift) - 1) >> sample_shift) * tile_rows + 63) / 64 * 64 : 0;
    if (sample_shift) t->d_skeys.reserve(t->reads, (size_t)sample_stride * gy);
    const size_t mirror_elems = bytes ? ((size_t)t->cap * t->dim + 1) / 2 : (size_t)t->cap * t->dim;  // in uint16 units
    t->mirror_rows = std::min(t->mirror_rows, t->rows);
    if (bytes && t->g8_ready && t->rows >= 4 * std::max<uint64_t>(t->g8_rows, 1)) t->g8_ready = false;  // the table has grown 4x since the
                                                                                    // channel scales were taken: look again
    if (bytes && !t->g8_ready) t->mirror_rows = 0;  // new scales: every byte row changes
    // the table grew past the mirror's allocation: the rows mirrored so far move over, only the new ones are converted
    const size_t keep_m = bytes ? ((size_t)t->mirror_rows * t->dim + 1) / 2 : (size_t)t->mirror_rows * t->dim;
    t->d_mirror.reserve_keep(t->reads, mirror_elems, keep_m);
    t->d_xx.reserve_keep(t->reads, (size_t)t->cap, (size_t)t->mirror_rows);
    if (bytes) {
        t->d_scale8.reserve_keep(t->reads, (size_t)t->cap, (size_t)t->mirror_rows);
        t->d_cfac8.reserve_keep(t->reads, (size_t)t->cap, (size_t)t->mirror_rows);
        t->d_rho8.reserve(t->reads, (size_t)KNN_GROUP_MAX);
        t->d_digits.reserve(t->reads, (size_t)KNN_GROUP_MAX * 3 * t->dim + 64);   // a group's queries as int8 digits
        t->d_qs.reserve(t->reads, (size_t)KNN_GROUP_MAX * 4);
        t->d_g8.reserve(t->reads, (size_t)2 * t->dim);
        if (!t->g8_ready) {  // the channel scales: RMS per dimension over a sample spread over the table (any positive values are correct)
            const uint64_t sample = std::min<uint64_t>(t->rows, 1u << 16), stride = t->rows / sample;
            HIP_CHECK(hipMemsetAsync(t->d_g8 + t->dim, 0, t->dim * sizeof(float), s));
            hipLaunchKernelGGL(knn_channel_sumsq_kernel, dim3(256), dim3(256), 0, s, t->table, sample, stride, (int)t->dim, t->d_g8 + t->dim);
            hipLaunchKernelGGL(knn_channel_scale_kernel, dim3((t->dim + 255) / 256), dim3(256), 0, s, t->d_g8 + t->dim, sample,
                               (int)t->dim, t->d_g8);
            t->g8_ready = true;
            t->g8_rows = t->rows;
        }
    }
    const uint64_t n_tiles = (t->rows + 63) / 64;
    const uint32_t blocks = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 4, (n_tiles + 3) / 4));
    // (a group multiplies the grid by its queries: fewer blocks per query then, or every one of 16 x 2048 blocks pays the
    // histogram pick of the previous pass — a 2048-bin scan — for a few iterations of work)
    const uint32_t hb1 = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 8, (t->rows + 255) / 256);
    const uint32_t hb = std::max<uint32_t>(std::min<uint32_t>(hb1, (uint32_t)t->n_cu), (hb1 + gy - 1) / gy);
    uint32_t* flags = t->d_pref_flag;  // {candidate count, fallback, go}; not in d_sel: the selects below clear that
    uint32_t* key32 = t->d_pref_rows + PREF_CAP;
    uint32_t* count2 = t->d_sel + 6 * SEL_BINS;
    SelState* states = reinterpret_cast<SelState*>(t->d_sel + 6 * SEL_BINS + 4);
    const size_t sel_bytes = (size_t)SEL_WORDS * gy * sizeof(uint32_t);
    HIP_CHECK(hipMemsetAsync(t->d_sel, 0, sel_bytes, s));
    HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)4 * gy * sizeof(uint32_t), s));
    static const uint32_t ring8_bpc = [] { const char* e = std::getenv("MI_KNN_RING_BPC"); return e ? (uint32_t)std::max(1, std::atoi(e)) : 2u; }();  // A/B
    const float e0 = 4.1f * (float)(t->dim + 8) * 0x1p-24f + 2e-6f;  // fp32 summations, norms, divisions
    const float eps = 0x1p-8f + e0;                                  // bf16: 8 significant bits, unit roundoff 2^-8
    // deleted rows: behind stage 1 their keys (and sampled keys) become 0xFFFFFFFF; the collect leaves them out
    const uint64_t* tomb = tomb_of(t);
    auto kill_keys = [&] {
        if (!tomb) return;
        const uint32_t nd = (uint32_t)t->dead.size();
        hipLaunchKernelGGL(knn_tomb_keys_kernel, dim3(std::max(1u, std::min<uint32_t>((nd + 255) / 256, (uint32_t)t->n_cu * 4))), dim3(256), 0, s,
                           t->d_dead, nd, t->rows, t->d_keys32, (uint64_t)t->cap, gy, sample_shift ? t->d_skeys : (uint32_t*)nullptr,
                           sample_stride, sample_shift, tile_rows);
    };
    if (bytes) {
        uint8_t* m8 = reinterpret_cast<uint8_t*>(t->d_mirror.p);
        const uint32_t* keys_q = t->d_keys32;   // query y: + y * cap (QGroup)
        // what the histogram passes read: every key, or the sample (its own stride between the queries of a group)
        const uint32_t* keys_h = sample_shift ? t->d_skeys : keys_q;
        const uint64_t n_h = sample_shift ? n_sample : t->rows;
        QGroup qgh = qg;
        if (sample_shift && gy > 1) qgh.keys = sample_stride;
        const uint32_t hbh = sample_shift ? std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>(hb, (n_h + 1023) / 1024)) : hb;
        switch (t->dim / 64) {
#define MI_CASE(NCH)                                                                                                     \
    case NCH:                                                                                                            \
        if (t->mirror_rows < t->rows) {                                                                                  \
            const uint64_t todo = t->rows - t->mirror_rows;                                                              \
            const uint32_t mb = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 8, (todo + 15) / 16);                   \
            hipLaunchKernelGGL((knn_mirror8_kernel<NCH>), dim3(std::max(mb, 1u)), dim3(256), 0, s, t->table, t->mirror_rows, \
                               t->rows, t->d_g8, m8, t->d_xx, t->d_scale8, t->d_cfac8);                                  \
            t->mirror_rows = t->rows;                                                                                    \
        }                                                                                                                \
        if (nq_batch == 0 && t->coarse_ring == 8)  /* 169 VGPRs: two workgroups per CU are resident, launch exactly those */ \
            hipLaunchKernelGGL((knn_scan_coarse8_kernel<NCH, 8>), dim3(std::min(blocks, (uint32_t)t->n_cu * ring8_bpc)), dim3(256), 0, s, m8, t->d_xx, t->d_scale8, \
                               t->d_cfac8, t->d_g8, t->rows, d_q, e0, t->d_keys32, t->d_rho8,                            \
                               sample_shift ? t->d_skeys : (uint32_t*)nullptr, sample_shift);                            \
        else if (nq_batch == 0)                                                                                          \
            hipLaunchKernelGGL((knn_scan_coarse8_kernel<NCH, 4>), dim3(blocks), dim3(256), 0, s, m8, t->d_xx, t->d_scale8, \
                               t->d_cfac8, t->d_g8, t->rows, d_q, e0, t->d_keys32, t->d_rho8,                            \
                               sample_shift ? t->d_skeys : (uint32_t*)nullptr, sample_shift);                            \
        else                                                                                                             \
            launch_coarse8_batched<NCH>(t, m8, d_q, e0, nq_batch, blocks, s, sample_shift, sample_stride);               \
        kill_keys();                                                                                                     \
        for (int p = 0; p < 3; ++p)                                                                                      \
            hipLaunchKernelGGL(knn_select_hist_kernel, dim3(hbh, gy), dim3(256), 0, s, keys_h, n_h, k, p, t->d_sel, states, \
                               (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, qgh, 0);    \
        hipLaunchKernelGGL(knn_prefilter_collect8_kernel, dim3(hb, gy), dim3(256), 0, s, keys_q, t->d_cfac8, t->rows, k, \
                           t->d_sel, states, t->d_rho8, e0, PREF_CAP, t->d_pref_rows, flags, qg, tomb);                  \
        hipLaunchKernelGGL((knn_rescore_kernel<NCH>), dim3(t->n_cu * (gy > 1 ? 2 : 8), gy), dim3(256), 0, s, t->table, d_q, \
                           t->d_pref_rows, flags, PREF_CAP, key32, qg);                                                  \
        break;
            MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
            default: fail(MI_ERR_UNSUPPORTED, "dim %u: the byte prefilter is built for dim/64 in {4,8,12,16}", t->dim);
        }
    } else
    switch (t->dim / 64) {
#define MI_CASE(NCH)                                                                                                     \
    case NCH:                                                                                                            \
        if (t->mirror_rows < t->rows) {                                                                                  \
            const uint64_t todo = t->rows - t->mirror_rows;                                                              \
            const uint32_t mb = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 8, (todo + 15) / 16);                   \
            hipLaunchKernelGGL((knn_mirror_kernel<NCH>), dim3(std::max(mb, 1u)), dim3(256), 0, s, t->table, t->mirror_rows, \
                               t->rows, t->d_mirror, t->d_xx);                                                           \
            t->mirror_rows = t->rows;                                                                                    \
        }                                                                                                                \
        hipLaunchKernelGGL((knn_scan_coarse_kernel<NCH>), dim3(blocks), dim3(256), 0, s, t->d_mirror, t->d_xx, t->rows,  \
                           d_q, t->d_keys32);                                                                            \
        kill_keys();                                                                                                     \
        for (int p = 0; p < 3; ++p)                                                                                      \
            hipLaunchKernelGGL(knn_select_hist_kernel, dim3(hb), dim3(256), 0, s, t->d_keys32, t->rows, k, p, t->d_sel, states); \
        hipLaunchKernelGGL(knn_prefilter_collect_kernel, dim3(hb), dim3(256), 0, s, t->d_keys32, t->rows, k, t->d_sel,   \
                           states, 2.0f * eps, PREF_CAP, t->d_pref_rows, flags, tomb);                                   \
        hipLaunchKernelGGL((knn_rescore_kernel<NCH>), dim3(t->n_cu * 8), dim3(256), 0, s, t->table, d_q, t->d_pref_rows, \
                           flags, PREF_CAP, key32);                                                                      \
        break;
        MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
        default: fail(MI_ERR_UNSUPPORTED, "dim %u: the prefilter is built for dim/64 in {2,4,8,12,16}", t->dim);
    }
    // the k smallest (exact key, row) pairs of the candidates: the radix select over the two arrays, unless there were too many
    HIP_CHECK(hipMemsetAsync(t->d_sel, 0, sel_bytes, s));
    const uint32_t* go = flags + 2;
    const uint32_t cb = (uint32_t)t->n_cu * 2;
    for (int p = 0; p < 6; ++p)
        hipLaunchKernelGGL(knn_select_hist_kernel, dim3(cb, gy), dim3(256), 0, s, key32, (uint64_t)PREF_CAP, k, p, t->d_sel, states, go, flags,
                           t->d_pref_rows, qg, 1);
    hipLaunchKernelGGL(knn_select_collect_kernel, dim3(cb, gy), dim3(256), 0, s, key32, (uint64_t)PREF_CAP, k, t->d_sel, states, t->d_cand, count2,
                       go, flags, t->d_pref_rows, qg, 1);
    hipLaunchKernelGGL(knn_select_sort_kernel, dim3(1, gy), dim3(1024), 0, s, t->d_cand, count2, k, t->d_pref_keys, go, qg);
    HIP_CHECK(hipGetLastError());
    return flags + 1;
}

// 64 < k <= 4096: every row's distance key, then the k smallest (distance, id) keys by radix select (knn_kernels.h)
// gy > 1: a group of gy queries (contiguous at d_q) in the same launches: query y gated by run_if[4 y], keys to keys_out + 4096 y
void select_pass(mi_knn* t, const float* d_q, uint32_t k, uint64_t* keys_out, hipStream_t s, const uint32_t* run_if = nullptr, uint32_t gy = 1) {
    const QGroup qg = group_of(t, gy);
    const uint64_t n_tiles = (t->rows + 63) / 64;
    uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 4, (n_tiles + 3) / 4);
    blocks = std::max(blocks, 1u);
    t->d_keys32.reserve(t->reads, (size_t)t->cap * gy);
    t->d_sel.reserve(t->reads, (size_t)SEL_WORDS * gy);
    t->d_cand.reserve(t->reads, (size_t)4096 * gy);
    HIP_CHECK(hipMemsetAsync(t->d_sel, 0, (size_t)SEL_WORDS * gy * sizeof(uint32_t), s));
    const uint64_t* tomb = tomb_of(t);
    const uint64_t n_dead = t->dead.size();
    switch (t->dim / 64) {
#define MI_CASE(NCH)                                                                                          \
    case NCH:                                                                                                 \
        hipLaunchKernelGGL((knn_scan_kernel<NCH, WaveTopReg, 1>), dim3(blocks, gy), dim3(256), 0, s, t->table, t->rows, d_q, k, \
                           (const uint64_t*)nullptr, (uint64_t*)nullptr, t->d_keys32, run_if, qg);            \
        break;
        MI_CASE(1) MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
        default: fail(MI_ERR_UNSUPPORTED, "dim %u: built for dim/64 in {1,2,4,8,12,16}", t->dim);
    }
    HIP_CHECK(hipGetLastError());
    // deleted rows: the scan above is the one a table without deletions runs; their keys then become 0xFFFFFFFF (O(deleted)
    // work) and the selects below leave those keys out
    if (tomb) {
        const uint32_t nd = (uint32_t)t->dead.size();
        hipLaunchKernelGGL(knn_tomb_keys_kernel, dim3(std::max(1u, std::min<uint32_t>((nd + 255) / 256, (uint32_t)t->n_cu * 4))), dim3(256), 0, s,
                           t->d_dead, nd, t->rows, t->d_keys32, (uint64_t)t->cap, gy, (uint32_t*)nullptr, (uint64_t)0, 0, 64u);
        HIP_CHECK(hipGetLastError());
    }
    const uint32_t hb = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 8, (t->rows + 255) / 256);
    uint32_t* count = t->d_sel + 6 * SEL_BINS;
    SelState* states = reinterpret_cast<SelState*>(t->d_sel + 6 * SEL_BINS + 4);  // 6 states of 24 bytes behind the counter
    for (int p = 0; p < 6; ++p)
        hipLaunchKernelGGL(knn_select_hist_kernel, dim3(hb, gy), dim3(256), 0, s, t->d_keys32, t->rows, k, p, t->d_sel, states, run_if,
                           (const uint32_t*)nullptr, (const uint32_t*)nullptr, qg, 0, tomb, n_dead);
    hipLaunchKernelGGL(knn_select_collect_kernel, dim3(hb, gy), dim3(256), 0, s, t->d_keys32, t->rows, k, t->d_sel, states, t->d_cand, count, run_if,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, qg, 0, tomb, n_dead);
    hipLaunchKernelGGL(knn_select_sort_kernel, dim3(1, gy), dim3(1024), 0, s, t->d_cand, count, k, keys_out, run_if, qg);
    HIP_CHECK(hipGetLastError());
}

// ---- feedback of the two-stage search (handles.h: pref_*) -------------------------------------------------------
void pref_window(mi_knn* t) {
    t->pref_skip_left = mi_knn::PREF_SKIP;
    t->pref_consec = 0;
    t->pref_probing = false;
}
void pref_fold(mi_knn* t, uint32_t cand, uint32_t fell_back) {
    t->pref_consec = fell_back ? t->pref_consec + 1 : 0;
    if (t->pref_probing) {  // the two probes behind a skip window: both must have reported before anything is decided
        if (t->pref_reports_due && --t->pref_reports_due == 0) {
            if (t->pref_consec >= 2) pref_window(t);
            else t->pref_probing = false;
        }
        return;
    }
    // (only fallbacks count: a search that re-evaluates even two million rows — 2.7 ms over 10 M rows — still beats the single
    // pass; a rule on the candidate count, tried first, sent such corpora to the slower path)
    (void)cand;
    if (t->pref_consec >= 2) pref_window(t);
}
// fold what has arrived, oldest first, without waiting for anything
void pref_poll(mi_knn* t) {
    for (uint64_t q = t->pref_seq >= (uint64_t)mi_knn::PREF_RING ? t->pref_seq - mi_knn::PREF_RING : 0; q < t->pref_seq; ++q) {
        const int i = (int)(q % mi_knn::PREF_RING);
        if (!t->pref_ev_pending[i]) continue;
        if (hipEventQuery(t->pref_ev[i]) != hipSuccess) { (void)hipGetLastError(); break; }  // keep the order: stop at the first one still in flight
        t->pref_ev_pending[i] = false;
        pref_fold(t, t->h_pref_ring.as<uint32_t>()[2 * i], t->h_pref_ring.as<uint32_t>()[2 * i + 1]);
    }
}
// behind a two-stage search on `s`: {candidates, fell back} -> pinned memory, an event to say when
void pref_record(mi_knn* t, hipStream_t s) {
    t->h_pref_ring.reserve((size_t)mi_knn::PREF_RING * 2 * sizeof(uint32_t));
    const int i = (int)(t->pref_seq % mi_knn::PREF_RING);
    if (t->pref_ev_pending[i]) {  // eight readbacks still in flight: this query goes unreported rather than waited for
        if (t->pref_probing && t->pref_reports_due && --t->pref_reports_due == 0) t->pref_probing = false;
        return;
    }
    t->pref_ev[i].get(hipEventDisableTiming);
    HIP_CHECK(hipMemcpyAsync(t->h_pref_ring.as<uint32_t>() + 2 * i, t->d_pref_flag, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(t->pref_ev[i], s));
    t->pref_ev_pending[i] = true;
    ++t->pref_seq;
}
void pref_reset(mi_knn* t) {
    for (int i = 0; i < mi_knn::PREF_RING; ++i) {
        if (t->pref_ev_pending[i]) (void)hipEventSynchronize(t->pref_ev[i]);
        t->pref_ev_pending[i] = false;
    }
    t->pref_consec = t->pref_skip_left = 0;
    t->pref_probing = false;
    t->pref_probes_left = t->pref_reports_due = 0;
}

// lists a register-path pass writes (the grid of one_pass<WaveTopReg>)
uint32_t reg_pass_lists(const mi_knn* t) {
    const uint64_t n_tiles = (t->rows + 63) / 64;
    return 4 * std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 4, (n_tiles + 3) / 4));
}

// One query (nq_batch = 0) or a group of nq_batch queries, contiguous at d_q, through the two stages; results to
// d_idx / d_dist [nq][k].  d_keys is sized by the caller (4096 keys per query).
void two_stage(mi_knn* t, const float* d_q, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s, uint32_t nq_batch) {
    const uint32_t gy = std::max(1u, nq_batch);
    const QGroup qg = group_of(t, gy);
    // every workspace of this search at its final size BEFORE the first launch: growing one later would free a buffer
    // that kernels already queued on `s` still use (reserve() only waits for EARLIER searches)
    if (k <= 64) {
        const uint32_t lists = reg_pass_lists(t);
        t->d_cand.reserve(t->reads, std::max<size_t>((size_t)4096 * gy, (size_t)lists * k * gy));
        if (lists > 64) t->d_tmp.reserve(t->reads, (size_t)((lists + 31) / 32) * k * gy);
    }
    const uint32_t* fallback = prefilter_pass(t, d_q, k, s, nq_batch);
    // the single pass, every kernel of it returning at once unless the query's fallback word is set
    if (k <= 64) one_pass<WaveTopReg>(t, d_q, k, nullptr, t->d_keys, s, fallback, gy, qg);
    else select_pass(t, d_q, k, t->d_keys, s, fallback, gy);
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, gy), dim3(256), 0, s, t->d_keys, k, knn_id_map(t),
                       d_idx, d_dist, (size_t)qg.out, (size_t)(gy > 1 ? k : 0), t->d_pref_keys, fallback, qg.flags);
    HIP_CHECK(hipGetLastError());
}

// nq = 2, 4 or 8 queries (contiguous at d_q) through the two stages with ONE pass over the byte mirror and ONE launch of
// every later kernel for the whole group (grid.y = query); bit-identical to nq single searches (the per-(row, query)
// arithmetic of stage 1 is the single kernel's; the selects and stage 2 are the single search's own kernels)
// A group counts as ONE search in the feedback of the two-stage search (handles.h: pref_*): it reports its first query's
// {candidates, fell back} words, it is one of the two probes behind a skip window, and a group of k <= 64 that is sent to
// the batched single pass instead counts the window down (k > 64 goes through search_one per query, which counts itself).
bool batched_two_stage_applies(mi_knn* t, uint32_t k) {
    if (!(t->prefilter == 2 && t->dim == 768 && prefilter_applies(t, k))) return false;
    if (!t->pref_adaptive) return true;
    pref_poll(t);
    if (t->pref_skip_left) {
        if (k <= 64) {
            if (--t->pref_skip_left == 0) { t->pref_probing = true; t->pref_probes_left = t->pref_reports_due = 2; t->pref_consec = 0; }
            ++t->pref_skipped;
        }
        return false;
    }
    if (t->pref_probing) {
        if (t->pref_probes_left) { --t->pref_probes_left; return true; }
        if (k <= 64) ++t->pref_skipped;
        return false;
    }
    return true;
}
void search_batched_two_stage(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    t->d_keys.reserve(t->reads, (size_t)4096 * nq);
    t->last_prefiltered = true;
    two_stage(t, d_q, k, d_idx, d_dist, s, nq);
    if (t->pref_adaptive) pref_record(t, s);   // the group's first query speaks for it (d_pref_flag[0..1])
}

void search_one(mi_knn* t, const float* d_q, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    if (t->rows == 0) {  // nothing stored: k "none" entries
        hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, 1), dim3(256), 0, s,
                           (const uint64_t*)nullptr, k, knn_id_map(t), d_idx, d_dist, (size_t)0, (size_t)0);
        HIP_CHECK(hipGetLastError());
        return;
    }
    const uint32_t passes = (k + 1023) / 1024;
    t->d_keys.reserve(t->reads, (size_t)std::max<uint32_t>(passes * 1024, 4096));
    t->last_prefiltered = prefilter_applies(t, k);
    if (t->last_prefiltered && t->pref_adaptive) {
        pref_poll(t);
        if (t->pref_skip_left) {  // this corpus has been defeating the mirror: the single pass alone, for a while
            if (--t->pref_skip_left == 0) { t->pref_probing = true; t->pref_probes_left = t->pref_reports_due = 2; t->pref_consec = 0; }
            ++t->pref_skipped;
            t->last_prefiltered = false;
        } else if (t->pref_probing) {
            if (t->pref_probes_left) --t->pref_probes_left;             // one of the two probes
            else { ++t->pref_skipped; t->last_prefiltered = false; }    // their reports are still on the way
        }
    }
    if (t->last_prefiltered) {
        two_stage(t, d_q, k, d_idx, d_dist, s, 0);
        if (t->pref_adaptive) pref_record(t, s);
        return;
    }
    // a table with deleted rows takes the radix select for k <= 64 too: the scan with the bitmap in it (knn_scan_kernel
    // TOMB) measured 13 % slower than the plain scan the select path runs
    if ((k > 64 || tomb_of(t)) && k <= 4096 && t->select_path) {
        select_pass(t, d_q, k, t->d_keys, s);
        hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, 1), dim3(256), 0, s, t->d_keys, k, knn_id_map(t),
                           d_idx, d_dist, (size_t)0, (size_t)0);
        HIP_CHECK(hipGetLastError());
        return;
    }
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t kp = std::min(1024u, k - p * 1024);
        uint64_t* out = t->d_keys + (size_t)p * 1024;
        const uint64_t* lo = p ? out - 1 : nullptr;  // last key of the previous pass
        if (kp <= 64) one_pass<WaveTopReg>(t, d_q, kp, lo, out, s);
        else if (kp <= 256) one_pass<WaveTopLds<256>>(t, d_q, kp, lo, out, s);
        else one_pass<WaveTopLds<1024>>(t, d_q, kp, lo, out, s);
    }
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, 1), dim3(256), 0, s, t->d_keys, k, knn_id_map(t),
                       d_idx, d_dist, (size_t)0, (size_t)0);
    HIP_CHECK(hipGetLastError());
}

template <int NQ>
void launch_batched(mi_knn* t, const float* d_q, uint32_t k, uint64_t* cand, uint32_t blocks, hipStream_t s) {
    switch (t->dim / 64) {
        case 12:
            if (const uint64_t* tomb = tomb_of(t))
                hipLaunchKernelGGL((knn_scan_batched_kernel<12, NQ, true>), dim3(blocks), dim3(256), 0, s, t->table, t->rows,
                                   d_q, k, cand, tomb);
            else
                hipLaunchKernelGGL((knn_scan_batched_kernel<12, NQ>), dim3(blocks), dim3(256), 0, s, t->table, t->rows,
                                   d_q, k, cand);
            break;
        default: fail(MI_ERR_UNSUPPORTED, "batched search is built for dim 768 (got %u)", t->dim);
    }
    HIP_CHECK(hipGetLastError());
}

// nq in {2,4,8} queries, k <= 64, one table pass
void search_batched(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist,
                    hipStream_t s) {
    const uint64_t n_tiles = (t->rows + 63) / 64;
    uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 2, (n_tiles + 3) / 4);
    blocks = std::max(blocks, 1u);
    const uint32_t lists = blocks * 4;
    t->d_cand.reserve(t->reads, (size_t)nq * lists * k);
    t->d_keys.reserve(t->reads, (size_t)std::max<uint32_t>(1024, nq * k));
    if (nq == 2) launch_batched<2>(t, d_q, k, t->d_cand, blocks, s);
    else if (nq == 4) launch_batched<4>(t, d_q, k, t->d_cand, blocks, s);
    else launch_batched<8>(t, d_q, k, t->d_cand, blocks, s);
    const size_t cstride = (size_t)lists * k;
    if (lists <= 64) {
        launch_merge<WaveTopReg>(t->d_cand, lists, k, lists, t->d_keys, nq, cstride, k, s);
    } else {
        const uint32_t lpb = 32, mid = (lists + lpb - 1) / lpb;
        t->d_tmp.reserve(t->reads, (size_t)nq * mid * k);
        launch_merge<WaveTopReg>(t->d_cand, lists, k, lpb, t->d_tmp, nq, cstride, (size_t)mid * k, s);
        launch_merge<WaveTopReg>(t->d_tmp, mid, k, mid, t->d_keys, nq, (size_t)mid * k, k, s);
    }
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, nq), dim3(256), 0, s, t->d_keys, k, knn_id_map(t),
                       d_idx, d_dist, (size_t)k, (size_t)k);
    HIP_CHECK(hipGetLastError());
}

void check_search_args(const mi_knn* t, const void* q, uint32_t nq, uint32_t k, const void* idx, const void* dist) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (nq && (!q || !idx || !dist)) fail(MI_ERR_INVALID, "null query/result pointer");
    if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
}

// nq queries on the device (contiguous at d_q), in groups that share their passes: up to 16 per group through the two-stage
// search over the byte mirror, else 8 / 4 / 2 over the fp32 rows (k <= 64), else one by one; results [nq][k]
void search_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    uint32_t u = 0;
    while (u < nq) {
        const uint32_t left = nq - u;
        if (left >= 2 && t->rows && batched_two_stage_applies(t, k)) {  // one pass over the byte mirror serves a group of up to 16 queries
            const uint32_t b2 = group_size(t, left);
            search_batched_two_stage(t, d_q + (size_t)u * t->dim, b2, k, d_idx + (size_t)u * k, d_dist + (size_t)u * k, s);
            u += b2;
            continue;
        }
        const uint32_t b = (k <= 64 && t->rows && t->dim == 768) ? (left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1) : 1;
        if (b == 1) search_one(t, d_q + (size_t)u * t->dim, k, d_idx + (size_t)u * k, d_dist + (size_t)u * k, s);
        else search_batched(t, d_q + (size_t)u * t->dim, b, k, d_idx + (size_t)u * k, d_dist + (size_t)u * k, s);
        u += b;
    }
}

// ---- filtered search (mi_knn_search_filtered): the k nearest among chosen rows ------------------------------------------
// The filter goes to the device as its live local rows, ascending (t->d_flist); knn_scan_gather_kernel reads only those rows.
constexpr uint32_t FILTER_K_MAX = 4096;

// room for `want` rows in the pinned host list (its old contents are not kept; nothing in flight reads it: every filtered
// entry point has waited for its results before it returned)
uint32_t* flist_reserve(mi_knn* t, size_t want) {
    t->h_flist.reserve(std::max(want, (size_t)4096) * sizeof(uint32_t));
    return t->h_flist.as<uint32_t>();
}

// ids -> t->h_flist [0, n_flist): the local rows they name, ascending, once each, deleted rows left out; MI_ERR_INVALID (and
// the list untouched) when an id is not a row of the table
void filter_rows(mi_knn* t, const uint64_t* ids, uint64_t n_ids) {
    std::vector<uint32_t> rows = knn_local_rows(t, ids, n_ids);
    // From rows / 1024 ids on, a bitmap over the rows (zeroed, marked, emitted: O(rows / 64 + n_ids)) instead of a sort
    // (O(n_ids log n_ids)): at 10 M rows the sort took 4 ms for 10^5 scattered ids and 570 ms for 10^7.
    if (n_ids >= t->rows / 1024) {
        std::vector<uint64_t> bits((size_t)((t->rows + 63) / 64), 0ull);
        for (const uint32_t r : rows) bits[r >> 6] |= 1ull << (r & 63);
        for (const uint32_t r : t->dead)
            if (r < t->rows) bits[r >> 6] &= ~(1ull << (r & 63));
        size_t n = 0;
        for (const uint64_t b : bits) n += (size_t)__builtin_popcountll(b);
        uint32_t* out = flist_reserve(t, n);
        size_t at = 0;
        for (size_t w = 0; w < bits.size(); ++w)
            for (uint64_t b = bits[w]; b; b &= b - 1) out[at++] = (uint32_t)(w * 64 + (uint64_t)__builtin_ctzll(b));
        t->n_flist = n;
        return;
    }
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    uint32_t* out = flist_reserve(t, rows.size());
    t->n_flist = (size_t)(std::set_difference(rows.begin(), rows.end(), t->dead.begin(), t->dead.end(), out) - out);
}

// grid of a gathered pass over n entries (as one_pass over n rows)
uint32_t gather_blocks(const mi_knn* t, uint32_t n, uint32_t bpc) {
    const uint64_t n_tiles = ((uint64_t)n + 63) / 64;
    return std::max(1u, (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * bpc, (n_tiles + 3) / 4));
}

// the kp <= 1024 smallest keys of the n entries, ascending, into keys_out: per-wave lists (Top) and the single pass's merge tree
template <class Top>
void gather_lists(mi_knn* t, const float* d_q, uint32_t n, uint32_t kp, uint64_t* keys_out, hipStream_t s) {
    const uint32_t blocks = gather_blocks(t, n, Top::LDS_KEYS == 0 ? 4 : (Top::KP <= 256 ? 4 : 2)), lists = blocks * 4;
    t->d_cand.reserve(t->reads, (size_t)lists * kp);
    const size_t lds = (size_t)4 * Top::LDS_KEYS * sizeof(uint64_t);
    switch (t->dim / 64) {
#define MI_CASE(NCH)                                                                                                    \
    case NCH:                                                                                                           \
        allow_lds(knn_scan_gather_kernel<NCH, Top>, lds);                                                               \
        hipLaunchKernelGGL((knn_scan_gather_kernel<NCH, Top>), dim3(blocks), dim3(256), lds, s, t->table, t->d_flist, n, d_q, kp, \
                           t->d_cand, (uint32_t*)nullptr);                                                              \
        break;
        MI_CASE(1) MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
        default: fail(MI_ERR_UNSUPPORTED, "dim %u: built for dim/64 in {1,2,4,8,12,16}", t->dim);
    }
    HIP_CHECK(hipGetLastError());
    QGroup qg;
    qg.lists = (uint64_t)lists * kp;
    reduce_wave_lists<Top>(t, lists, kp, keys_out, s, nullptr, 1, qg);
}

// the radix select over the n compact keys in t->d_keys32 with the entry's position as the low word (t->d_sel zeroed, t->d_cand
// holds 4096 keys); list (nullable): positions back to rows afterwards
void select_keys32(mi_knn* t, uint64_t n, uint32_t k, uint64_t* keys_out, const uint32_t* list, hipStream_t s) {
    const uint32_t hb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)t->n_cu * 8, (n + 255) / 256));
    uint32_t* count = t->d_sel + 6 * SEL_BINS;
    SelState* states = reinterpret_cast<SelState*>(t->d_sel + 6 * SEL_BINS + 4);
    for (int p = 0; p < 6; ++p)
        hipLaunchKernelGGL(knn_select_hist_kernel, dim3(hb), dim3(256), 0, s, t->d_keys32, n, k, p, t->d_sel, states);
    hipLaunchKernelGGL(knn_select_collect_kernel, dim3(hb), dim3(256), 0, s, t->d_keys32, n, k, t->d_sel, states, t->d_cand, count);
    hipLaunchKernelGGL(knn_select_sort_kernel, dim3(1), dim3(1024), 0, s, t->d_cand, count, k, keys_out);
    if (list) hipLaunchKernelGGL(knn_gather_rows_kernel, dim3((k + 255) / 256), dim3(256), 0, s, keys_out, k, list);
    HIP_CHECK(hipGetLastError());
}

// the k <= 4096 smallest keys of the n entries, ascending, into keys_out: one distance key per entry, the radix select over
// (key, position), then positions back to rows
void gather_select(mi_knn* t, const float* d_q, uint32_t n, uint32_t k, uint64_t* keys_out, hipStream_t s) {
    t->d_keys32.reserve(t->reads, (size_t)n);
    t->d_sel.reserve(t->reads, (size_t)SEL_WORDS);
    t->d_cand.reserve(t->reads, (size_t)4096);
    HIP_CHECK(hipMemsetAsync(t->d_sel, 0, (size_t)SEL_WORDS * sizeof(uint32_t), s));
    const uint32_t blocks = gather_blocks(t, n, 4);
    switch (t->dim / 64) {
#define MI_CASE(NCH)                                                                                                    \
    case NCH:                                                                                                           \
        hipLaunchKernelGGL((knn_scan_gather_kernel<NCH, WaveTopReg, 1>), dim3(blocks), dim3(256), 0, s, t->table, t->d_flist, n, \
                           d_q, k, (uint64_t*)nullptr, t->d_keys32);                                                    \
        break;
        MI_CASE(1) MI_CASE(2) MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16)
#undef MI_CASE
        default: fail(MI_ERR_UNSUPPORTED, "dim %u: built for dim/64 in {1,2,4,8,12,16}", t->dim);
    }
    HIP_CHECK(hipGetLastError());
    select_keys32(t, n, k, keys_out, t->d_flist, s);
}

// Per-wave lists or the radix select for 64 < k <= 1024: the lists pay while a wave sees many more entries than k (most of
// its offers then fail the threshold test); near k entries per wave nearly everything passes and the merge tree of
// waves x k keys costs more than the select's passes over n compact keys.  Rule: lists when every wave of the full grid
// sees at least 16 k entries (k = 100: n >= 3.3 M entries on 256 CUs).  A handle made with MI_KNN_SELECT=0 (the single
// pass's A/B hook) takes the lists for every k <= 1024.  The lists are WaveTopLds<1024> for every 64 < k <= 1024: the gathered
// scan with WaveTopLds<256> takes 154 VGPRs at dim 768 (3 waves per SIMD against the 4 of knn_scan_kernel<12, WaveTopLds<256>>,
// and 112 bytes of scratch when held to 4); with WaveTopLds<1024> it takes 160 VGPRs, the 3 waves of the scan's own form.
bool filter_takes_lists(const mi_knn* t, uint32_t n, uint32_t k) {
    if (k <= 64) return true;
    if (k > 1024) return false;
    if (!t->select_path) return true;
    const uint64_t waves = 4ull * t->n_cu * 2;
    return (uint64_t)n >= 16ull * k * waves;
}

void filtered_one(mi_knn* t, const float* d_q, uint32_t n, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    if (n == 0) {  // nothing qualifies: k "none" entries
        hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, 1), dim3(256), 0, s, (const uint64_t*)nullptr, k, knn_id_map(t),
                           d_idx, d_dist, (size_t)0, (size_t)0);
        HIP_CHECK(hipGetLastError());
        return;
    }
    t->d_keys.reserve(t->reads, (size_t)FILTER_K_MAX);
    if (!filter_takes_lists(t, n, k)) gather_select(t, d_q, n, k, t->d_keys, s);
    else if (k <= 64) gather_lists<WaveTopReg>(t, d_q, n, k, t->d_keys, s);
    else gather_lists<WaveTopLds<1024>>(t, d_q, n, k, t->d_keys, s);
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, 1), dim3(256), 0, s, t->d_keys, k, knn_id_map(t), d_idx, d_dist,
                       (size_t)0, (size_t)0);
    HIP_CHECK(hipGetLastError());
}

// nq in {2, 4, 8} queries over one filter, k <= 64, dim 768: one gathered pass (knn_scan_gather_batched_kernel)
void filtered_batched(mi_knn* t, const float* d_q, uint32_t nq, uint32_t n, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    const uint32_t blocks = gather_blocks(t, n, 2), lists = blocks * 4;
    t->d_cand.reserve(t->reads, (size_t)nq * lists * k);
    t->d_keys.reserve(t->reads, (size_t)std::max<uint32_t>(FILTER_K_MAX, nq * k));
    if (nq == 2)
        hipLaunchKernelGGL((knn_scan_gather_batched_kernel<12, 2>), dim3(blocks), dim3(256), 0, s, t->table, t->d_flist, n, d_q, k, t->d_cand);
    else if (nq == 4)
        hipLaunchKernelGGL((knn_scan_gather_batched_kernel<12, 4>), dim3(blocks), dim3(256), 0, s, t->table, t->d_flist, n, d_q, k, t->d_cand);
    else
        hipLaunchKernelGGL((knn_scan_gather_batched_kernel<12, 8>), dim3(blocks), dim3(256), 0, s, t->table, t->d_flist, n, d_q, k, t->d_cand);
    HIP_CHECK(hipGetLastError());
    const size_t cstride = (size_t)lists * k;
    if (lists <= 64) {
        launch_merge<WaveTopReg>(t->d_cand, lists, k, lists, t->d_keys, nq, cstride, k, s);
    } else {
        const uint32_t lpb = 32, mid = (lists + lpb - 1) / lpb;
        t->d_tmp.reserve(t->reads, (size_t)nq * mid * k);
        launch_merge<WaveTopReg>(t->d_cand, lists, k, lpb, t->d_tmp, nq, cstride, (size_t)mid * k, s);
        launch_merge<WaveTopReg>(t->d_tmp, mid, k, mid, t->d_keys, nq, (size_t)mid * k, k, s);
    }
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((k + 255) / 256, nq), dim3(256), 0, s, t->d_keys, k, knn_id_map(t), d_idx, d_dist,
                       (size_t)k, (size_t)k);
    HIP_CHECK(hipGetLastError());
}

// the list to the device, once per call, from pinned memory (untouched until the call has waited for its results)
void upload_filter(mi_knn* t, hipStream_t s) {
    const size_t n = t->n_flist;
    if (n == 0) return;
    t->d_flist.reserve(t->reads, n);
    HIP_CHECK(hipMemcpyAsync(t->d_flist, t->h_flist.p, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
}

// nq queries (contiguous at d_q) over the uploaded filter, in groups of 8 / 4 / 2 (k <= 64, dim 768) or one by one
void filtered_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    const uint32_t n = (uint32_t)t->n_flist;
    uint32_t u = 0;
    while (u < nq) {
        const uint32_t left = nq - u;
        const uint32_t b = (k <= 64 && n && t->dim == 768) ? (left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1) : 1;
        if (b == 1) filtered_one(t, d_q + (size_t)u * t->dim, n, k, d_idx + (size_t)u * k, d_dist + (size_t)u * k, s);
        else filtered_batched(t, d_q + (size_t)u * t->dim, b, n, k, d_idx + (size_t)u * k, d_dist + (size_t)u * k, s);
        u += b;
    }
}
}  // namespace

namespace mi {
void knn_search_filtered_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, const uint64_t* ids, uint64_t n_ids,
                              uint64_t* d_idx, float* d_dist, hipStream_t s) {
    filter_rows(t, ids, n_ids);
    upload_filter(t, s);
    filtered_many(t, d_q, nq, k, d_idx, d_dist, s);
}
IdMap knn_id_map(const mi_knn* t) { return IdMap{t->base, t->cyc_block, t->cyc_n, t->cyc_rank}; }
std::vector<uint32_t> knn_local_rows(const mi_knn* t, const uint64_t* ids, uint64_t n) {
    if (!ids && n > t->rows) fail(MI_ERR_INVALID, "%llu rows asked of a table of %llu", (unsigned long long)n, (unsigned long long)t->rows);
    std::vector<uint32_t> rows((size_t)n);
    const IdMap m = knn_id_map(t);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t local = i;
        if (ids && !local_of_id(m, t->rows, ids[i], &local))
            fail(MI_ERR_INVALID, "id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)ids[i],
                 (unsigned long long)t->base, (unsigned long long)t->rows);
        rows[(size_t)i] = (uint32_t)local;
    }
    return rows;
}
hipStream_t knn_own_stream(mi_knn* t) { return own_stream(t); }
void knn_filter_rows(mi_knn* t, const uint64_t* ids, uint64_t n_ids) { filter_rows(t, ids, n_ids); }
void knn_filter_upload(mi_knn* t, hipStream_t s) { upload_filter(t, s); }
void knn_filtered_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    filtered_many(t, d_q, nq, k, d_idx, d_dist, s);
}
void knn_reduce_lists64(mi_knn* t, uint32_t lists, uint32_t k, uint64_t* keys_out, hipStream_t s) {
    QGroup qg;
    qg.lists = (uint64_t)lists * k;
    reduce_wave_lists<WaveTopReg>(t, lists, k, keys_out, s, nullptr, 1, qg);
}
void knn_select_keys32(mi_knn* t, uint64_t n, uint32_t k, uint64_t* keys_out, const uint32_t* list, hipStream_t s) {
    t->d_sel.reserve(t->reads, (size_t)SEL_WORDS);
    t->d_cand.reserve(t->reads, (size_t)4096);
    HIP_CHECK(hipMemsetAsync(t->d_sel, 0, (size_t)SEL_WORDS * sizeof(uint32_t), s));
    select_keys32(t, n, k, keys_out, list, s);
}
void knn_search_many(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    search_many(t, d_q, nq, k, d_idx, d_dist, s);
}
void knn_grow(mi_knn* t, uint64_t want_rows) { grow(t, want_rows); }
// the group column (grouped.hip): one id per row of capacity, the rows it gains hold MI_KNN_NO_GROUP (all ones)
void knn_groups_fit(mi_knn* t) { fit(t, std::max<size_t>((size_t)t->cap, 64), t->d_groups.fill, t->d_groups); }
// the attribute columns (where.hip): 64 flags and one ordered value per row of capacity, the rows they gain hold 0 / 0
void knn_attrs_fit(mi_knn* t) { fit(t, std::max<size_t>((size_t)t->cap, 64), t->d_tags.fill, t->d_tags, t->d_stamps); }
void knn_search_one(mi_knn* t, const float* d_q, uint32_t k, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    search_one(t, d_q, k, d_idx, d_dist, s);
}
void knn_truncate(mi_knn* t, uint64_t rows) {
    std::lock_guard<std::mutex> l(t->mu);
    if (rows >= t->rows) return;
    t->rows = rows;
    t->mirror_rows = std::min(t->mirror_rows, rows);
    // ... and what their columns held (a later append reuses those rows, without a group and with the default attributes)
    if (t->d_groups || t->d_tags) {
        DeviceGuard g(t->device);
        t->writes.sync();
        t->reads.sync();
        if (t->d_groups) {
            for (size_t r = (size_t)rows; r < t->d_groups.host.size(); ++r) t->n_grouped -= t->d_groups.host[r] != MI_KNN_NO_GROUP;
            ++t->groups_epoch;
        }
        hipStream_t s = own_stream(t);
        t->d_groups.truncate((size_t)rows, s);
        t->d_tags.truncate((size_t)rows, s);
        t->d_stamps.truncate((size_t)rows, s);
        HIP_CHECK(hipStreamSynchronize(s));
    }
    // the rows beyond are forgotten, their tombstones with them (a later append reuses those rows, live)
    const auto cut = std::lower_bound(t->dead.begin(), t->dead.end(), (uint32_t)std::min<uint64_t>(rows, 0xFFFFFFFFull));
    if (cut != t->dead.end()) {
        t->dead.erase(cut, t->dead.end());
        DeviceGuard g(t->device);
        tomb_rebuild(t);
    }
}
void knn_merge_lists_device(const uint64_t* d_idx_in, const float* d_dist_in, uint32_t lists, uint32_t nq, uint32_t k,
                            size_t idx_stride, size_t dist_stride, uint64_t* d_idx, float* d_dist, hipStream_t s) {
    const uint32_t threads = std::max<uint32_t>(lists * k, k);
    for (uint32_t u0 = 0; u0 < nq; u0 += 65535) {  // grid.y holds 65535 queries
        const uint32_t nu = std::min<uint32_t>(65535, nq - u0);
        hipLaunchKernelGGL(knn_merge_lists_kernel, dim3((threads + 255) / 256, nu), dim3(256), 0, s, d_idx_in + (size_t)u0 * k,
                           d_dist_in + (size_t)u0 * k, lists, k, idx_stride, dist_stride, d_idx + (size_t)u0 * k, d_dist + (size_t)u0 * k);
        HIP_CHECK(hipGetLastError());
    }
}
}  // namespace mi

extern "C" {

int mi_knn_create(uint32_t dim, int device, mi_knn** out) {
    return guarded([&] {
        if (!out) fail(MI_ERR_INVALID, "out is null");
        *out = nullptr;
        if (dim == 0 || dim % 64 != 0) fail(MI_ERR_UNSUPPORTED, "dim must be a positive multiple of 64 (got %u)", dim);
        DeviceGuard g(device);
        std::unique_ptr<mi_knn> t(new mi_knn());   // whatever fails below, what it owns by then goes with it
        t->device = device; t->dim = dim;
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        t->n_cu = prop.multiProcessorCount;
        t->d_q.alloc((size_t)16 * dim);
        if (const char* e = std::getenv("MI_KNN_SELECT")) t->select_path = std::atoi(e) != 0;  // A/B hook, read at creation
        if (const char* e = std::getenv("MI_KNN_RING")) t->coarse_ring = std::atoi(e) == 8 ? 8 : 4;
        if (const char* e = std::getenv("MI_KNN_BATCH_STAGE1")) t->batch_stage1_mfma = std::atoi(e) != 0;  // A/B hook, read at creation
        *out = t.release();
    });
}

void mi_knn_free(mi_knn* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    t->stream.reset();
    delete t;   // the workspace, the columns, the pinned buffers and the events go with their owners
}

int mi_knn_set_option(mi_knn* t, const char* key, int value) {
    return guarded([&] {
        if (!t || !key) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        const std::string k(key);
        if (k == "prefilter") {
            // two-stage exact search: a mirror of the rows (1: bf16, + 50 % memory; 2: bytes, + 25 %; built by the next search
            // and kept up to date by every later one) prefilters, the fp32 rows decide; results are those of the single pass
            if (value < 0 || value > 2) fail(MI_ERR_INVALID, "prefilter: 0, 1 or 2 (got %d)", value);
            if (value != t->prefilter && t->d_mirror) {  // another form (or none): the mirror goes, the next search rebuilds
                DeviceGuard g(t->device);
                t->reads.sync();
                t->d_mirror.release();
                t->d_xx.release();
                t->d_scale8.release();
                t->d_cfac8.release();
                t->mirror_rows = 0;
                t->g8_ready = false;
            }
            if (value != t->prefilter) pref_reset(t);
            t->prefilter = value;
        } else if (k == "prefilter_sample") {
            // 1 (default): a GROUP of queries, k <= 64, over the byte mirror takes the collect threshold from a sample of the stage-1
            // keys (an eighth of the select's reads, a few times more rows for stage 2); 2: single queries too; 0: always from all
            // keys.  Same answers either way.
            if (value < 0 || value > 2) fail(MI_ERR_INVALID, "prefilter_sample must be 0, 1 or 2");
            t->pref_sample = value;
        } else if (k == "batch_stage1") {
            // 1 (default): the shared stage 1 of a group of queries on the matrix pipe (int8 MFMA, knn_scan_coarse8_mfma_kernel);
            // 0: the vector-ALU form (knn_scan_coarse8_batched_kernel).  Same answers either way.
            t->batch_stage1_mfma = value != 0;
        } else if (k == "prefilter_adaptive") {
            // 1 (default): a corpus that makes the two-stage search FALL BACK twice in a row is served by the single pass alone
            // for the next 64 single-query searches, then probed again with two queries (only fallbacks count: the candidate
            // count does not, pref_fold); 0: every query tries stage 1
            pref_reset(t);
            t->pref_adaptive = value != 0;
        } else if (k == "join_cap") {
            // candidate pairs one strip of mi_knn_near_pairs' first stage may hand to its second (default 2^22; at least one
            // full tile, 2^14): a strip that finds more is redone in smaller pieces.  Same answers whatever the value.
            if (value < (1 << 14)) fail(MI_ERR_INVALID, "join_cap must be >= 16384 (got %d)", value);
            t->join_cap = (uint32_t)value;
        } else if (k == "join_stage") {
            // mi_knn_near_pairs_between / mi_knn_sharded_near_pairs with this table as the row side: 1 = the column side goes
            // through the staged copy even when it lives on this table's device (what a column side on another device always
            // takes); 0 (default): it is read where it lies.  Same answers either way.
            if (value < 0 || value > 1) fail(MI_ERR_INVALID, "join_stage must be 0 or 1 (got %d)", value);
            t->join_stage = value;
        } else if (k == "join_stage_rows") {
            // ... rows of one column chunk (staged or read where it lies), rounded up to whole tiles of 128.  0 (default): what
            // the staging budget (256 MiB of fp32 rows) holds.  Same answers whatever the value.
            if (value < 0) fail(MI_ERR_INVALID, "join_stage_rows must be >= 0 (got %d)", value);
            t->join_stage_rows = value;
        } else if (k == "many_segments") {
            // mi_knn_search_many / mi_knn_neighbors: column segments of a stage-1 launch.  0 (default): from the query and column
            // tile counts; v >= 1: exactly min(v, column tiles).  Same answers whatever the value.
            if (value < 0) fail(MI_ERR_INVALID, "many_segments must be >= 0 (got %d)", value);
            t->many_segments = value;
        } else if (k == "many_sample") {
            // ... the threshold pass visits every v-th column tile.  0 (default): chosen by the table's size; 1: every tile.
            // Same answers whatever the value (a sparser sample hands stage 2 more candidates).
            if (value < 0) fail(MI_ERR_INVALID, "many_sample must be >= 0 (got %d)", value);
            t->many_sample = value;
        } else if (k == "kmeans_fixed_sum") {
            // mi_knn_kmeans' update and mi_knn_summarize's centroids: 0 (default) = the float sums in the order the row ids fix;
            // 1 = exact integer sums of 2^-30 (assign_kernels.h), the arithmetic mi_knn_sharded_kmeans always takes: a sharded
            // table holding the same rows then returns the same bits.
            if (value < 0 || value > 1) fail(MI_ERR_INVALID, "kmeans_fixed_sum must be 0 or 1 (got %d)", value);
            t->kmeans_fixed_sum = value;
        } else if (k == "compound_blocks") {
            // mi_knn_search_compound: workgroups of its scan.  0 (default): the grid the batched search takes; v >= 1: exactly
            // min(v, tiles / 4) — a small table can then make a wave walk several tiles.  Same answers whatever the value.
            if (value < 0) fail(MI_ERR_INVALID, "compound_blocks must be >= 0 (got %d)", value);
            t->compound_blocks = value;
        } else if (k == "page_blocks") {
            // mi_knn_search_page: workgroups of its scan, the rule of "compound_blocks".  0 (default): the single pass's grid;
            // v >= 1: exactly min(v, tiles / 4).  Same answers whatever the value.
            if (value < 0) fail(MI_ERR_INVALID, "page_blocks must be >= 0 (got %d)", value);
            t->page_blocks = value;
        } else if (k == "group_blocks") {
            // mi_knn_search_grouped: workgroups of its reduce and mark passes.  0 (default): four per CU; v >= 1: exactly
            // min(v, keys / 256).  Same answers whatever the value.
            if (value < 0) fail(MI_ERR_INVALID, "group_blocks must be >= 0 (got %d)", value);
            t->group_blocks = value;
        } else if (k == "group_lds_max") {
            // ... the largest n_groups whose reduce pass builds block-private tables in LDS (12 bytes per group; default and
            // maximum 4096 = 48 KiB, two workgroups per CU); above it, and with 0 always, the pass works on the global slots.
            // Same answers whatever the value.
            if (value < 0 || value > 4096) fail(MI_ERR_INVALID, "group_lds_max must be in [0, 4096] (got %d)", value);
            t->group_lds_max = value;
        } else if (k == "where_chunk") {
            // mi_knn_search_where and its kin: rows one workgroup of the predicate passes owns.  0 (default): 4096; otherwise a
            // multiple of 64 up to 65536.  Same answers whatever the value.
            if (!where_chunk_ok(value)) fail(MI_ERR_INVALID, "where_chunk must be 0 or a multiple of 64 up to 65536 (got %d)", value);
            t->where_chunk = value;
        } else if (k == "compact_chunk_rows") {
            // mi_knn_compact: destination rows of one chunk of its in-place move (and of its staging buffer).  0 (default): what
            // 64 MiB hold of rows of this dim (21 845 at dim 768).  Same table afterwards whatever the value.
            if (value < 0) fail(MI_ERR_INVALID, "compact_chunk_rows must be >= 0 (got %d)", value);
            t->compact_chunk_rows = value;
        } else {
            fail(MI_ERR_INVALID, "unknown option '%s' (known: prefilter, prefilter_adaptive, prefilter_sample, batch_stage1, join_cap, join_stage, join_stage_rows, many_segments, many_sample, kmeans_fixed_sum, compound_blocks, page_blocks, group_blocks, group_lds_max, where_chunk, compact_chunk_rows)", key);
        }
    });
}

int mi_knn_prefilter_stats(mi_knn* t, uint32_t* candidates, uint32_t* fell_back) {
    return guarded([&] {
        if (!t || !candidates || !fell_back) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        *candidates = 0; *fell_back = 0;
        if (!t->last_prefiltered) return;
        DeviceGuard g(t->device);
        t->reads.sync();
        uint32_t w[2] = {0, 0};
        HIP_CHECK(hipMemcpy(w, t->d_pref_flag, sizeof w, hipMemcpyDeviceToHost));
        *candidates = w[0]; *fell_back = w[1];
    });
}

int mi_knn_prefilter_state(mi_knn* t, uint32_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        t->reads.sync();   // everything enqueued has finished, so every readback has arrived
        pref_poll(t);
        out[0] = t->pref_skip_left;
        out[1] = t->pref_consec;
        out[2] = (uint32_t)std::min<uint64_t>(t->pref_skipped, 0xFFFFFFFFull);
        out[3] = (uint32_t)std::min<uint64_t>(t->g8_rows, 0xFFFFFFFFull);
    });
}

int mi_knn_set_base(mi_knn* t, uint64_t base) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        std::lock_guard<std::mutex> l(t->mu);
        t->base = base;
    });
}

int mi_knn_reserve(mi_knn* t, uint64_t rows) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        grow(t, rows);
    });
}

int mi_knn_size(const mi_knn* t, uint64_t* rows) {
    return guarded([&] {
        if (!t || !rows) fail(MI_ERR_INVALID, "null argument");
        *rows = t->rows;
    });
}

int mi_knn_append(mi_knn* t, const float* rows, uint64_t n) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        if (!rows) fail(MI_ERR_INVALID, "rows is null");
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        own_stream(t);
        grow(t, t->rows + n);
        t->writes.begin(t->stream);
        HIP_CHECK(hipMemcpyAsync(t->table + t->rows * t->dim, rows, n * t->dim * sizeof(float), hipMemcpyHostToDevice,
                                 t->stream));
        t->writes.end(t->stream);
        HIP_CHECK(hipStreamSynchronize(t->stream));
        t->rows += n;
    });
}

int mi_knn_append_device(mi_knn* t, const float* d_rows, uint64_t n, void* stream) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        if (!d_rows) fail(MI_ERR_INVALID, "d_rows is null");
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        hipStream_t s = stream ? (hipStream_t)stream : own_stream(t);
        grow(t, t->rows + n);  // a reallocation waits for the handle's work in flight and copies synchronously
        t->writes.begin(s);
        HIP_CHECK(hipMemcpyAsync(t->table + t->rows * t->dim, d_rows, n * t->dim * sizeof(float),
                                 hipMemcpyDeviceToDevice, s));
        // `rows` counts the new rows from now on; a search on any stream waits for this event first
        t->writes.end(s);
        t->rows += n;
    });
}

int mi_knn_append_synthetic(mi_knn* t, uint64_t seed, uint64_t first_row, uint64_t n) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        own_stream(t);
        grow(t, t->rows + n);
        const uint64_t key = [&] {  // synth.py: mix64(seed + GOLDEN)
            uint64_t z = seed + 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        }();
        const float scale = (float)(1.0 / std::sqrt(1431655765.0));
        hipLaunchKernelGGL(gen_f32_kernel, dim3(t->n_cu * 8), dim3(256), 0, t->stream, t->table + t->rows * t->dim,
                           key, first_row * t->dim, n * t->dim, scale);
        HIP_CHECK(hipGetLastError());
        t->writes.end(t->stream);
        HIP_CHECK(hipStreamSynchronize(t->stream));
        t->rows += n;
    });
}

int mi_knn_get_rows(mi_knn* t, uint64_t first, uint64_t n, float* out) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (n == 0) return;
        if (!out) fail(MI_ERR_INVALID, "out is null");
        std::lock_guard<std::mutex> l(t->mu);
        if (first + n > t->rows) fail(MI_ERR_INVALID, "rows [%llu,%llu) out of range (size %llu)",
                                      (unsigned long long)first, (unsigned long long)(first + n),
                                      (unsigned long long)t->rows);
        DeviceGuard g(t->device);
        own_stream(t);
        t->writes.begin(t->stream);
        HIP_CHECK(hipMemcpyAsync(out, t->table + first * t->dim, n * t->dim * sizeof(float), hipMemcpyDeviceToHost,
                                 t->stream));
        HIP_CHECK(hipStreamSynchronize(t->stream));
    });
}

// ---- deleted rows: DELETE FROM image WHERE id IN $ids (what the reference's database does for a removed image) ----
int mi_knn_delete(mi_knn* t, const uint64_t* ids, uint64_t n, uint64_t* newly) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (newly) *newly = 0;
        if (n == 0) return;
        if (!ids) fail(MI_ERR_INVALID, "ids is null");
        std::lock_guard<std::mutex> l(t->mu);
        // every id is checked before anything changes: a call with one bad id deletes nothing
        std::vector<uint32_t> rows = knn_local_rows(t, ids, n);
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        std::vector<uint32_t> fresh;
        std::set_difference(rows.begin(), rows.end(), t->dead.begin(), t->dead.end(), std::back_inserter(fresh));
        if (fresh.empty()) return;  // already deleted: nothing to do
        DeviceGuard g(t->device);
        hipStream_t s = own_stream(t);
        // a write that changes what searches read: it waits for the searches enqueued before it (any stream), and every
        // search enqueued after it waits for it (writes)
        t->writes.begin(s);
        t->reads.begin(s);
        tomb_add(t, fresh, s);
        t->writes.end(s);
        HIP_CHECK(hipStreamSynchronize(s));
        if (newly) *newly = fresh.size();
    });
}

int mi_knn_deleted(mi_knn* t, uint64_t* ids, uint64_t cap, uint64_t* count) {
    return guarded([&] {
        if (!t || !count) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        *count = t->dead.size();
        if (!ids) return;
        const IdMap m = knn_id_map(t);  // monotone in the local row: ascending rows give ascending ids
        for (uint64_t i = 0; i < std::min<uint64_t>(cap, t->dead.size()); ++i) ids[i] = id_of_local(m, t->dead[i]);
    });
}

// ---- persistence of a shard: what SurrealDB's storage does for
// `image.embedding` (server/src/clip.rs:125-137).  File = 32-byte header {"MIKNNv01", u32 dim,
// u32 reserved, u64 rows, u64 base} + rows*dim little-endian f32, streamed through a 64 MiB
// pinned buffer so that neither side needs the table in host memory.  A table with deleted rows writes "MIKNNv02":
// the same header and rows, then u64 count + count u64 local rows, ascending (an older library refuses such a file
// instead of bringing the deleted rows back); without deletions the file is the MIKNNv01 file, byte for byte.
namespace {
struct KnnFileHeader { char magic[8]; uint32_t dim, reserved; uint64_t rows, base; };
static_assert(sizeof(KnnFileHeader) == 32, "header layout");
constexpr size_t IO_CHUNK = 64u << 20;
struct File {
    FILE* f;
    File(const char* path, const char* mode) : f(std::fopen(path, mode)) {}
    ~File() { if (f) std::fclose(f); }
};
}  // namespace

int mi_knn_save(mi_knn* t, const char* path) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (!path) fail(MI_ERR_INVALID, "path is null");
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        own_stream(t);
        // crash-safe: everything goes to `<path>.tmp`, is flushed and fsync'ed, and only then renamed over
        // `path` — a full disk or a crash leaves the previous file, never a truncated one that reports success
        const std::string tmp = std::string(path) + ".tmp";
        {
            File f(tmp.c_str(), "wb");
            if (!f.f) fail(MI_ERR_IO, "cannot create %s", tmp.c_str());
            KnnFileHeader h{};
            std::memcpy(h.magic, t->dead.empty() ? "MIKNNv01" : "MIKNNv02", 8);
            h.dim = t->dim; h.rows = t->rows; h.base = t->base;
            if (std::fwrite(&h, sizeof h, 1, f.f) != 1) fail(MI_ERR_IO, "write to %s failed", tmp.c_str());
            const size_t total = (size_t)t->rows * t->dim * sizeof(float);
            if (total) {
                PinnedBuf buf(std::min(total, IO_CHUNK), hipHostMallocDefault);
                t->writes.begin(t->stream);
                for (size_t off = 0; off < total; off += IO_CHUNK) {
                    const size_t n = std::min(IO_CHUNK, total - off);
                    HIP_CHECK(hipMemcpyAsync(buf.p, (const char*)t->table.p + off, n, hipMemcpyDeviceToHost, t->stream));
                    HIP_CHECK(hipStreamSynchronize(t->stream));
                    if (std::fwrite(buf.p, 1, n, f.f) != n) fail(MI_ERR_IO, "write to %s failed (disk full?)", tmp.c_str());
                }
            }
            if (!t->dead.empty()) {
                const uint64_t cnt = t->dead.size();
                std::vector<uint64_t> rows(t->dead.begin(), t->dead.end());
                if (std::fwrite(&cnt, 8, 1, f.f) != 1 || std::fwrite(rows.data(), 8, rows.size(), f.f) != rows.size())
                    fail(MI_ERR_IO, "write to %s failed (disk full?)", tmp.c_str());
            }
            if (std::fflush(f.f) != 0 || fsync(fileno(f.f)) != 0) fail(MI_ERR_IO, "flush of %s failed", tmp.c_str());
            FILE* fp = f.f;
            f.f = nullptr;
            if (std::fclose(fp) != 0) fail(MI_ERR_IO, "close of %s failed", tmp.c_str());
        }
        if (std::rename(tmp.c_str(), path) != 0) fail(MI_ERR_IO, "cannot rename %s to %s", tmp.c_str(), path);
        {   // the rename becomes durable with its directory
            const std::string p(path);
            const size_t slash = p.find_last_of('/');
            File d((slash == std::string::npos ? std::string(".") : slash == 0 ? std::string("/") : p.substr(0, slash)).c_str(), "r");
            if (d.f) (void)fsync(fileno(d.f));
        }
    });
}

int mi_knn_load(mi_knn* t, const char* path) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (!path) fail(MI_ERR_INVALID, "path is null");
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        own_stream(t);
        File f(path, "rb");
        if (!f.f) fail(MI_ERR_IO, "cannot open %s", path);
        KnnFileHeader h{};
        if (std::fread(&h, sizeof h, 1, f.f) != 1 || (std::memcmp(h.magic, "MIKNNv01", 8) != 0 && std::memcmp(h.magic, "MIKNNv02", 8) != 0))
            fail(MI_ERR_IO, "%s is not a MIKNNv01 / MIKNNv02 shard file", path);
        const bool v2 = std::memcmp(h.magic, "MIKNNv02", 8) == 0;
        if (h.dim != t->dim) fail(MI_ERR_INVALID, "%s holds dim %u rows, the table has dim %u", path, h.dim, t->dim);
        if (t->rows == 0) t->base = h.base;  // an empty table takes the shard's id range
        else if (h.base != t->base + t->rows)
            fail(MI_ERR_INVALID, "%s starts at id %llu; the table (base %llu, %llu rows) would renumber its rows", path,
                 (unsigned long long)h.base, (unsigned long long)t->base, (unsigned long long)t->rows);
        const size_t total = (size_t)h.rows * t->dim * sizeof(float);
        if (total == 0) return;
        if (t->rows + h.rows > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "a shard holds at most 2^32-1 rows");
        grow(t, t->rows + h.rows);
        PinnedBuf buf(std::min(total, IO_CHUNK), hipHostMallocDefault);
        char* dst = (char*)(t->table + t->rows * t->dim);
        for (size_t off = 0; off < total; off += IO_CHUNK) {
            const size_t n = std::min(IO_CHUNK, total - off);
            if (std::fread(buf.p, 1, n, f.f) != n) fail(MI_ERR_IO, "%s is truncated", path);
            HIP_CHECK(hipMemcpyAsync(dst + off, buf.p, n, hipMemcpyHostToDevice, t->stream));
            HIP_CHECK(hipStreamSynchronize(t->stream));
        }
        // MIKNNv02: the file's deleted rows, read (and checked) before anything of the file counts
        std::vector<uint32_t> dead;
        if (v2) {
            uint64_t cnt = 0;
            if (std::fread(&cnt, 8, 1, f.f) != 1 || cnt > h.rows) fail(MI_ERR_IO, "%s: truncated or corrupt list of deleted rows", path);
            std::vector<uint64_t> rows((size_t)cnt);
            if (cnt && std::fread(rows.data(), 8, (size_t)cnt, f.f) != (size_t)cnt) fail(MI_ERR_IO, "%s is truncated", path);
            dead.reserve((size_t)cnt);
            for (uint64_t i = 0; i < cnt; ++i) {
                if (rows[i] >= h.rows || (i && rows[i] <= rows[i - 1])) fail(MI_ERR_IO, "%s: corrupt list of deleted rows", path);
                dead.push_back((uint32_t)(t->rows + rows[i]));  // the file's rows continue the table
            }
        }
        t->rows += h.rows;
        if (!dead.empty()) {
            tomb_add(t, dead, t->stream);
            HIP_CHECK(hipStreamSynchronize(t->stream));
        }
    });
}

int mi_knn_search_device(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx, float* d_dist,
                         void* stream) {
    return guarded([&] {
        check_search_args(t, d_q, nq, k, d_idx, d_dist);
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        hipStream_t s = stream ? (hipStream_t)stream : own_stream(t);
        t->writes.begin(s);
        t->reads.begin(s);
        for (uint32_t u = 0; u < nq; ++u)
            search_one(t, d_q + (size_t)u * t->dim, k, d_idx + (size_t)u * k, d_dist + (size_t)u * k, s);
        t->reads.end(s);
    });
}

int mi_knn_search_batched_device(mi_knn* t, const float* d_q, uint32_t nq, uint32_t k, uint64_t* d_idx,
                                 float* d_dist, void* stream) {
    return guarded([&] {
        check_search_args(t, d_q, nq, k, d_idx, d_dist);
        if (nq > 16) fail(MI_ERR_UNSUPPORTED, "batched search takes at most 16 queries (got %u)", nq);
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        hipStream_t s = stream ? (hipStream_t)stream : own_stream(t);
        t->writes.begin(s);
        t->reads.begin(s);
        search_many(t, d_q, nq, k, d_idx, d_dist, s);
        t->reads.end(s);
    });
}

// The merge every rank runs on what the all-gather left it, on the device: in = [lists][nq][k].
int mi_knn_merge_device(int device, const uint64_t* d_idx_in, const float* d_dist_in, uint32_t lists, uint32_t nq, uint32_t k,
                        uint64_t* d_idx, float* d_dist, void* stream) {
    return guarded([&] {
        if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
        if (nq == 0) return;
        if (!d_idx || !d_dist || (lists && (!d_idx_in || !d_dist_in))) fail(MI_ERR_INVALID, "null argument");
        if ((uint64_t)lists * k > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "lists * k too large");
        DeviceGuard g(device);
        knn_merge_lists_device(d_idx_in, d_dist_in, lists, nq, k, (size_t)nq * k, (size_t)nq * k, d_idx, d_dist, (hipStream_t)stream);
    });
}

int mi_knn_search(mi_knn* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] {
        check_search_args(t, q, nq, k, idx, dist);
        if (nq == 0) return;
        std::lock_guard<std::mutex> l(t->mu);
        DeviceGuard g(t->device);
        own_stream(t);
        // groups of up to 16 queries: one upload, table passes of 8 / 4 / 2 queries where the register
        // path applies (k <= 64; same arithmetic per query as the single-query pass), one readback
        constexpr uint32_t GROUP = 16;
        t->d_idx.reserve(t->reads, (size_t)GROUP * k);
        t->d_dist.reserve(t->reads, (size_t)GROUP * k);
        t->writes.begin(t->stream);
        t->reads.begin(t->stream);
        for (uint32_t u0 = 0; u0 < nq; u0 += GROUP) {
            const uint32_t ng = std::min(GROUP, nq - u0);
            HIP_CHECK(hipMemcpyAsync(t->d_q, q + (size_t)u0 * t->dim, (size_t)ng * t->dim * sizeof(float),
                                     hipMemcpyHostToDevice, t->stream));
            uint32_t u = 0;
            while (u < ng) {
                const uint32_t left = ng - u;
                if (left >= 2 && batched_two_stage_applies(t, k)) {
                    const uint32_t b2 = group_size(t, left);
                    search_batched_two_stage(t, t->d_q + (size_t)u * t->dim, b2, k, t->d_idx + (size_t)u * k, t->d_dist + (size_t)u * k, t->stream);
                    u += b2;
                    continue;
                }
                const uint32_t b = (k <= 64 && t->rows && t->dim == 768) ? (left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1) : 1;
                if (b == 1) search_one(t, t->d_q + (size_t)u * t->dim, k, t->d_idx + (size_t)u * k, t->d_dist + (size_t)u * k, t->stream);
                else search_batched(t, t->d_q + (size_t)u * t->dim, b, k, t->d_idx + (size_t)u * k, t->d_dist + (size_t)u * k, t->stream);
                u += b;
            }
            HIP_CHECK(hipMemcpyAsync(idx + (size_t)u0 * k, t->d_idx, (size_t)ng * k * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                     t->stream));
            HIP_CHECK(hipMemcpyAsync(dist + (size_t)u0 * k, t->d_dist, (size_t)ng * k * sizeof(float), hipMemcpyDeviceToHost,
                                     t->stream));
            HIP_CHECK(hipStreamSynchronize(t->stream));
        }
        t->reads.pending = false;
    });
}

// k nearest among the rows the ids name (WHERE embedding <|K|> $reference AND id IN $ids, a pre-filter): the result of a
// search over a table that holds only the filter's live rows under their own ids
int mi_knn_search_filtered(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const uint64_t* ids, uint64_t n_ids, uint64_t* idx,
                           float* dist) {
    return guarded([&] {
        check_search_args(t, q, nq, k, idx, dist);
        if (k > FILTER_K_MAX) fail(MI_ERR_UNSUPPORTED, "a filtered search takes k <= %u (got %u)", FILTER_K_MAX, k);
        if (n_ids && !ids) fail(MI_ERR_INVALID, "ids is null");
        std::lock_guard<std::mutex> l(t->mu);
        filter_rows(t, ids, n_ids);  // every id checked before anything runs
        if (nq == 0) return;
        DeviceGuard g(t->device);
        own_stream(t);
        constexpr uint32_t GROUP = 16;
        t->d_idx.reserve(t->reads, (size_t)GROUP * k);
        t->d_dist.reserve(t->reads, (size_t)GROUP * k);
        t->writes.begin(t->stream);
        t->reads.begin(t->stream);
        upload_filter(t, t->stream);
        for (uint32_t u0 = 0; u0 < nq; u0 += GROUP) {
            const uint32_t ng = std::min(GROUP, nq - u0);
            HIP_CHECK(hipMemcpyAsync(t->d_q, q + (size_t)u0 * t->dim, (size_t)ng * t->dim * sizeof(float),
                                     hipMemcpyHostToDevice, t->stream));
            filtered_many(t, t->d_q, ng, k, t->d_idx, t->d_dist, t->stream);
            HIP_CHECK(hipMemcpyAsync(idx + (size_t)u0 * k, t->d_idx, (size_t)ng * k * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                     t->stream));
            HIP_CHECK(hipMemcpyAsync(dist + (size_t)u0 * k, t->d_dist, (size_t)ng * k * sizeof(float), hipMemcpyDeviceToHost,
                                     t->stream));
            HIP_CHECK(hipStreamSynchronize(t->stream));
        }
        t->reads.pending = false;
    });
}

}  // extern "C"
