// search_many.hip — host side of mi_knn_search_many (the k <= 16 nearest live rows for each of nq query vectors), of
// mi_knn_neighbors (the same with the table's own rows as the queries: a slice of the kNN graph) and of
// mi_knn_sharded_search_many; and of the same calls narrowed by a predicate (mi_knn_search_many_where,
// mi_knn_neighbors_where, mi_knn_sharded_search_many_where) and of the vote built on them (mi_knn_propose_groups).  The
// kernels and the superset argument: search_many_kernels.h; the mask and the vote: search_many_where_kernels.h.
//
// The queries are walked in strips of at most STRIP_TILES row tiles.  A strip owns all per-query state: its fp32 queries
// and their bf16 mirror (mi_knn_search_many; mi_knn_neighbors reads both where they lie), the threshold slots of stage 1
// (4 m bytes per query), the key slots of stage 2 (8 m bytes) and the unpacked results (12 k bytes).  With the candidate
// buffer ("join_cap" pairs of 8 bytes) that is the device workspace beyond the table's mirror: it does not grow with nq.
// Per strip: one threshold pass, then the emit pass in pieces of row tiles sized so that a piece's candidates fit the
// buffer (from the rate the previous piece saw); a piece that overflows is redone in halves, query tiles first, then
// column ranges — only its emit pass: the strip's thresholds stay valid for every piece.
//
// A narrowed call builds a call-private bitmap "this row stays out" (many_mask_kernel) and hands it to stage 1 in place of
// the deletion bitmap, for the columns (col_mask) and, for the vote, for the query rows too (row_mask).  Nothing else in the
// walk changes, with one exception: when the unmasked columns times the strip's queries fit the candidate buffer, the
// threshold pass is skipped (the slots stay empty, so stage 1 emits every unmasked column for every query, in one piece that
// cannot overflow).  That also covers the small end of the masks whose rows fall into few residues mod m.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "search_many_kernels.h"
#include "search_many_where_kernels.h"
#include "sharded_call.h"
#include "two_stage.h"
#include "where_host.h"

using namespace mi;

namespace {

constexpr uint32_t STRIP_TILES = 512;   // query tiles of a strip (65 536 queries)
constexpr uint32_t MAX_K = 16;
constexpr uint32_t MAX_SEGMENTS = 65535;   // grid.y

// One call's state: the table's mirror (the columns), one strip's queries, slots and results on the device.
struct SearchMany {
    mi_knn* t = nullptr;
    hipStream_t s = nullptr;
    Scratch scratch;
    uint32_t n_cols = 0, m = 0, k = 0, n_cb = 0, cand_cap = 0, strip_rows = 0, sample = 1;
    bool self_drop = false;
    float thr = 0.0f;
    const uint16_t* mirror = nullptr;
    const float* xx = nullptr;
    const uint64_t* tomb = nullptr;   // the columns' bitmap: the table's deleted rows, or col_mask
    // a narrowed call (build_mask): the rows that may not answer / may not ask, `matched` = the columns left
    const uint64_t *dead = nullptr, *col_mask = nullptr, *row_mask = nullptr;
    uint64_t matched = 0;
    // mi_knn_propose_groups: the tally instead of the finalize kernel; results [rows] on the device
    bool vote = false;
    uint32_t hi_key = 0;
    uint32_t *d_vgroup = nullptr, *d_votes = nullptr, *d_heard = nullptr;
    float* d_vdist = nullptr;
    unsigned long long* d_vtotals = nullptr;
    uint32_t strips = 0;
    // the strip under way: n_s queries, fp32 and mirrored; for mi_knn_neighbors query r is the table's local row q_local0 + r
    const float* qf = nullptr;
    const uint16_t* qm = nullptr;
    const float* qx = nullptr;
    const uint64_t* q_tomb = nullptr;
    uint32_t q_local0 = 0, n_s = 0;
    float* d_qf = nullptr;           // [strip rows][dim] (mi_knn_search_many)
    uint16_t* d_qm = nullptr;
    float* d_qx = nullptr;
    uint2* d_cand = nullptr;
    unsigned long long *d_count = nullptr, *d_hits = nullptr, *d_slot = nullptr;
    int* d_gslot = nullptr;          // [strip rows][m]: stage 1's thresholds
    uint64_t* d_idx = nullptr;       // [strip rows][k]
    float* d_dist = nullptr;
    uint64_t stats[4] = {0, 0, 0, 0};

    // segments of a launch over n_rt row tiles and n_i column tiles: "many_segments" or enough that the workgroups are
    // several times the machine's slots, a segment not shorter than four tiles
    uint32_t segments(uint32_t n_rt, uint32_t n_i) const {
        uint32_t v = t->many_segments > 0 ? (uint32_t)t->many_segments
                                          : std::min<uint32_t>(((uint32_t)t->n_cu * 16 + n_rt - 1) / n_rt, std::max(1u, n_i / 4));
        return std::max(1u, std::min({v, n_i, MAX_SEGMENTS}));
    }

    template <int NCH, bool EMIT>
    void tiles(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t step, uint32_t n_i) {
        static DevOnce once;
        constexpr int LDS = EMIT ? SMY_LDS_EMIT : SMY_LDS_THR;
        allow_lds_once(once, search_many_tiles_kernel<NCH, EMIT>, LDS);
        hipLaunchKernelGGL((search_many_tiles_kernel<NCH, EMIT>), dim3(br1 - br0, segments(br1 - br0, n_i)), dim3(256), LDS, s, qm, qx,
                           q_tomb, q_local0, n_s, mirror, xx, tomb, n_cols, m, br0, bc0, step, n_i, thr, d_gslot, cand_cap, d_cand,
                           d_count);
        HIP_CHECK(hipGetLastError());
        ++stats[2];
        stats[3] += (uint64_t)(br1 - br0) * n_i;
    }

    // the emit pass of query tiles [br0, br1) x column tiles [bc0, bc1), and stage 2 of what it found
    template <int NCH>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) {
            HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
            tiles<NCH, true>(r0, r1, c0, 1, c1 - c0);
            return read_count(d_count, s);
        };
        auto stage2 = [&](uint32_t n) {   // (the queries' slots of stage 2 live in d_slot: they join the column pieces)
            stats[0] += n;
            hipLaunchKernelGGL((assign_multi_rescore_kernel<NCH>), dim3(group16_blocks(t, n)), dim3(256), 0, s, qf, t->table, d_cand, n,
                               m, __builtin_inff(), 0u, d_slot);
            HIP_CHECK(hipGetLastError());
        };
        rect_stages(br0, br1, bc0, bc1, cand_cap, overflowed, stage1, stage2);
    }

    // qf / qm / qx / q_tomb / q_local0 / n_s describe the strip -> idx / dist of its n_s queries on the host
    template <int NCH>
    void strip(uint64_t* idx, float* dist) {
        const size_t el = (size_t)n_s * m;
        HIP_CHECK(hipMemsetAsync(d_slot, 0xFF, el * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_gslot, TILE_ORD_NINF, el, s));
        const uint32_t n_rt = (n_s + TILE - 1) / TILE;
        // (a masked call whose every (query, column) pair fits the buffer: no thresholds, one piece)
        const bool all_at_once = col_mask && matched * n_s <= cand_cap;
        if (!all_at_once) tiles<NCH, false>(0, n_rt, 0, sample, (n_cb + sample - 1) / sample);
        uint32_t piece = all_at_once ? n_rt : std::max(1u, std::min(n_rt, cand_cap / (TILE * 16u * m)));
        ++strips;
        for (uint32_t br = 0; br < n_rt;) {
            const uint32_t end = std::min(n_rt, br + piece);
            const uint64_t before = stats[0];
            bool overflowed = false;
            rect<NCH>(br, end, 0, n_cb, &overflowed);
            // the next piece: half the buffer at the rate this one saw
            const uint64_t per_tile = (stats[0] - before) / (end - br) + 1;
            piece = overflowed ? std::max(1u, piece / 2) : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_rt, cand_cap / (2 * per_tile)));
            br = end;
        }
        if (vote) {
            hipLaunchKernelGGL(many_vote_kernel, dim3((n_s + 255) / 256), dim3(256), 0, s, d_slot, q_tomb, q_local0, n_s, m, hi_key,
                               t->d_groups, d_vgroup, d_votes, d_heard, d_vdist, d_vtotals);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));   // the strip's buffers are the next strip's
            return;
        }
        const IdMap map = knn_id_map(t);
        hipLaunchKernelGGL(search_many_finalize_kernel, dim3((n_s + 255) / 256), dim3(256), 0, s, d_slot, q_tomb, q_local0, n_s, m,
                           self_drop ? 1u : 0u, map, d_idx, d_dist, d_hits);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(idx, d_idx, (size_t)n_s * k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(dist, d_dist, (size_t)n_s * k * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));   // the strip's buffers are the next strip's
    }

    void strip(uint64_t* idx, float* dist) {
        dispatch_nch(t->dim, [&](auto nch) { strip<decltype(nch)::value>(idx, dist); });
    }

    // nq queries on the host -> idx / dist [nq][k]
    void run_queries(const float* q, uint32_t nq, uint64_t* idx, float* dist) {
        d_qf = (float*)scratch.get((size_t)strip_rows * t->dim * sizeof(float));
        d_qm = (uint16_t*)scratch.get((size_t)strip_rows * t->dim * sizeof(uint16_t));
        d_qx = (float*)scratch.get((size_t)strip_rows * sizeof(float));
        qf = d_qf; qm = d_qm; qx = d_qx; q_tomb = nullptr; q_local0 = 0;
        for (uint32_t q0 = 0; q0 < nq; q0 += strip_rows) {
            n_s = std::min(strip_rows, nq - q0);
            HIP_CHECK(hipMemcpyAsync(d_qf, q + (size_t)q0 * t->dim, (size_t)n_s * t->dim * sizeof(float), hipMemcpyHostToDevice, s));
            mirror_rows(t, s, d_qf, 0, n_s, d_qm, d_qx);
            strip(idx + (size_t)q0 * k, dist + (size_t)q0 * k);
        }
        finish();
    }

    // the table's local rows first .. first + n - 1 as the queries, read where they lie
    void run_rows(uint32_t first, uint32_t n, uint64_t* idx, float* dist) {
        q_tomb = row_mask ? row_mask : dead;
        for (uint32_t q0 = 0; q0 < n; q0 += strip_rows) {
            n_s = std::min(strip_rows, n - q0);
            q_local0 = first + q0;
            qf = t->table + (size_t)q_local0 * t->dim;
            qm = mirror + (size_t)q_local0 * t->dim;
            qx = xx + q_local0;
            if (vote) strip(nullptr, nullptr);
            else strip(idx + (size_t)q0 * k, dist + (size_t)q0 * k);
        }
        finish();
    }

    // the vote of every row (askers = the rows row_mask leaves): group / votes / heard / dist [rows] on the host (the last
    // three nullable), out[0 .. 2) = {rows with a proposal, rows whose voters all agree}
    void run_vote(uint32_t* group, uint32_t* votes, uint32_t* heard, float* dist, uint64_t out[2]) {
        const size_t n = n_cols;
        d_vgroup = (uint32_t*)scratch.get(n * sizeof(uint32_t));
        d_votes = votes ? (uint32_t*)scratch.get(n * sizeof(uint32_t)) : nullptr;
        d_heard = heard ? (uint32_t*)scratch.get(n * sizeof(uint32_t)) : nullptr;
        d_vdist = dist ? (float*)scratch.get(n * sizeof(float)) : nullptr;
        d_vtotals = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
        HIP_CHECK(hipMemsetAsync(d_vtotals, 0, 2 * sizeof(unsigned long long), s));
        run_rows(0, n_cols, nullptr, nullptr);   // (the strips write d_vgroup ... at their rows)
        unsigned long long got[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(got, d_vtotals, sizeof got, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(group, d_vgroup, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (votes) HIP_CHECK(hipMemcpyAsync(votes, d_votes, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (heard) HIP_CHECK(hipMemcpyAsync(heard, d_heard, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (dist) HIP_CHECK(hipMemcpyAsync(dist, d_vdist, n * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        out[0] = got[0]; out[1] = got[1];
        const uint64_t st[4] = {stats[0], stats[2], stats[3], strips};
        for (int i = 0; i < 4; ++i) t->propose_stats[i] = st[i];
    }

    // A bitmap of the rows that stay out (many_mask_kernel), enqueued; *d_clear (zeroed by the caller, on the stream) gains
    // the rows that take part.  open() first; the table not empty.
    void open(const TableCall& call) { t = call.t; s = call.s; }
    const uint64_t* build_mask(const WherePred& p, uint32_t rule, uint32_t x, unsigned long long* d_clear) {
        const uint64_t words = (t->rows + 63) / 64;
        uint64_t* mask = (uint64_t*)scratch.get((size_t)words * sizeof(uint64_t));
        hipLaunchKernelGGL(many_mask_kernel, dim3((uint32_t)((words + 3) / 4)), dim3(256), 0, s, p,
                           reinterpret_cast<const unsigned long long*>(t->d_tags.p), reinterpret_cast<const long long*>(t->d_stamps.p),
                           t->d_groups, t->dead.empty() ? nullptr : reinterpret_cast<const unsigned long long*>(t->d_tomb.p), t->rows,
                           rule, x, mask, d_clear);
        HIP_CHECK(hipGetLastError());
        return mask;
    }
    // the predicate as the columns' mask -> the qualifying rows (waits for the count)
    uint64_t mask_columns(const mi_knn_where& w) {
        unsigned long long* d_clear = (unsigned long long*)scratch.get(sizeof(unsigned long long));
        HIP_CHECK(hipMemsetAsync(d_clear, 0, sizeof(unsigned long long), s));
        col_mask = build_mask(pred_of(w), MASK_GROUP_ANY, 0u, d_clear);
        matched = read_count(d_clear, s);
        return matched;
    }

    void finish() {
        if (vote) return;
        unsigned long long hits = 0;
        HIP_CHECK(hipMemcpyAsync(&hits, d_hits, sizeof hits, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        stats[1] = hits;
        for (int i = 0; i < 4; ++i) t->search_many_stats[i] = stats[i];
    }

    // inside the call's frame (declared after this object: the stream is idle before the scratch memory goes); arguments
    // checked, the table not empty; nq = the queries of the call
    void setup(const TableCall& call, uint32_t nq, uint32_t n_keep, bool drop) {
        t = call.t;
        k = n_keep;
        self_drop = drop;
        m = k + (drop ? 1u : 0u);
        s = call.s;
        n_cols = (uint32_t)t->rows;
        n_cb = (n_cols + TILE - 1) / TILE;
        thr = 2.0f * eps2(t->dim);   // the join's bound, unchanged (join_kernels.h): both operands are rounded to bf16
        cand_cap = std::max<uint32_t>(TILE_CAP_MIN, t->join_cap);
        // the threshold pass visits every sample-th column tile ("many_sample"; by default all of them: DESIGN.md 5.18)
        sample = t->many_sample > 0 ? (uint32_t)t->many_sample : 1u;
        sample = std::max(1u, std::min(sample, n_cb));
        const TableMirror tm = table_mirror(t, s, scratch);
        mirror = tm.mirror; xx = tm.xx; dead = tm.tomb;
        tomb = col_mask ? col_mask : dead;
        strip_rows = (uint32_t)std::min<uint64_t>((uint64_t)STRIP_TILES * TILE, nq);
        const size_t strip_el = (size_t)strip_rows * m;
        d_cand = (uint2*)scratch.get((size_t)cand_cap * sizeof(uint2));
        d_count = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
        d_hits = d_count + 1;
        HIP_CHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), s));
        d_slot = (unsigned long long*)scratch.get(strip_el * sizeof(unsigned long long));
        d_gslot = (int*)scratch.get(strip_el * sizeof(int));
        if (vote) return;
        d_idx = (uint64_t*)scratch.get((size_t)strip_rows * k * sizeof(uint64_t));
        d_dist = (float*)scratch.get((size_t)strip_rows * k * sizeof(float));
    }
};

void check_table(const mi_knn* t) {
    check_mirror_dim(t->dim, "the");
    // (a shard never grows beyond this: the candidate record is a pair of uint32)
    if (t->rows > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "a shard holds at most 2^32-1 rows");
}

void check_args(const mi_knn* t, const float* q, uint32_t nq, uint32_t k, const uint64_t* idx, const float* dist) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (!q) fail(MI_ERR_INVALID, "q is null");
    if (!idx || !dist) fail(MI_ERR_INVALID, "idx / dist is null");
    if (nq == 0) fail(MI_ERR_INVALID, "nq must be >= 1");
    if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
    if (k > MAX_K) fail(MI_ERR_UNSUPPORTED, "at most %u neighbours per query (got %u)", MAX_K, k);
    check_table(t);
}

void pad(uint64_t* idx, float* dist, size_t n) {
    std::fill(idx, idx + n, MI_KNN_NO_ID);
    std::fill(dist, dist + n, INFINITY);
}

// the shard's answer, [nq][k], among the rows that qualify under w (null: the live rows, and then nothing but what
// mi_knn_search_many always ran); returns their number
uint64_t search_many_local(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w, uint64_t* idx, float* dist) {
    std::lock_guard<std::mutex> l(t->mu);
    for (uint64_t& v : t->search_many_stats) v = 0;
    if (t->rows == 0 || (w && where_never(*w, t->d_groups != nullptr))) {
        pad(idx, dist, (size_t)nq * k);
        return 0;
    }
    SearchMany a;
    TableCall call(t);
    if (w) {
        a.open(call);
        if (a.mask_columns(*w) == 0) {
            pad(idx, dist, (size_t)nq * k);
            return 0;
        }
    }
    a.setup(call, nq, k, false);
    a.run_queries(q, nq, idx, dist);
    return w ? a.matched : t->rows - t->dead.size();
}

void check_where(const mi_knn_where* w) {
    const char* why = "";
    const int bad = where_check_pred(w, &why);
    if (bad != MI_OK) fail(bad, "%s", why);
}

// mi_knn_neighbors / mi_knn_neighbors_where (w null: the former, launch for launch)
void neighbors(mi_knn* t, uint64_t first, uint64_t n, uint32_t k, const mi_knn_where* w, uint64_t* idx, float* dist) {
    if (!t) fail(MI_ERR_INVALID, "null table handle");
    if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
    if (k > MAX_K - 1) fail(MI_ERR_UNSUPPORTED, "at most %u neighbours per row (got %u)", MAX_K - 1, k);
    if (n != 0 && (!idx || !dist)) fail(MI_ERR_INVALID, "idx / dist is null");
    if (w) check_where(w);
    check_table(t);
    std::lock_guard<std::mutex> l(t->mu);
    if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "a shard of a sharded table holds no contiguous ids: use mi_knn_sharded_search_many");
    if (first < t->base || first - t->base > t->rows || n > t->rows - (first - t->base))
        fail(MI_ERR_INVALID, "rows [%llu,%llu) are not rows of this table (base %llu, %llu rows)", (unsigned long long)first,
             (unsigned long long)(first + n), (unsigned long long)t->base, (unsigned long long)t->rows);
    for (uint64_t& v : t->search_many_stats) v = 0;
    if (n == 0) return;
    if (w && where_never(*w, t->d_groups != nullptr)) {
        pad(idx, dist, (size_t)n * k);
        return;
    }
    SearchMany a;
    TableCall call(t);
    if (w) {
        a.open(call);
        if (a.mask_columns(*w) == 0) {
            pad(idx, dist, (size_t)n * k);
            return;
        }
    }
    a.setup(call, (uint32_t)n, k, true);
    a.run_rows((uint32_t)(first - t->base), (uint32_t)n, idx, dist);
}

WherePred every_live_row() {
    mi_knn_where w{};
    w.stamp_lo = INT64_MIN; w.stamp_hi = INT64_MAX;
    return pred_of(w);
}

}  // namespace

extern "C" {

int mi_knn_search_many(mi_knn* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] {
        check_args(t, q, nq, k, idx, dist);
        search_many_local(t, q, nq, k, nullptr, idx, dist);
    });
}

int mi_knn_search_many_where(mi_knn* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w, uint64_t* idx, float* dist,
                             uint64_t* matched) {
    return guarded([&] {
        if (w) check_where(w);   // (first: the predicate's own error is told even where something else is wrong too)
        check_args(t, q, nq, k, idx, dist);
        const uint64_t n = search_many_local(t, q, nq, k, w, idx, dist);
        if (matched) *matched = n;
    });
}

int mi_knn_search_many_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->search_many_stats[i];
    });
}

int mi_knn_neighbors(mi_knn* t, uint64_t first, uint64_t n, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] { neighbors(t, first, n, k, nullptr, idx, dist); });
}

int mi_knn_neighbors_where(mi_knn* t, uint64_t first, uint64_t n, uint32_t k, const mi_knn_where* w, uint64_t* idx, float* dist) {
    return guarded([&] { neighbors(t, first, n, k, w, idx, dist); });
}

int mi_knn_propose_groups(mi_knn* t, uint32_t k, float max_dist, uint32_t ask_group, const mi_knn_where* voters, uint32_t* group,
                          uint32_t* votes, uint32_t* heard, float* dist, uint64_t totals[4]) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (!group) fail(MI_ERR_INVALID, "group is null");
        if (k == 0) fail(MI_ERR_INVALID, "k must be >= 1");
        if (k > MAX_K) fail(MI_ERR_UNSUPPORTED, "at most %u voters per row (got %u)", MAX_K, k);
        if (!(max_dist >= 0.0f)) fail(MI_ERR_INVALID, "max_dist must be >= 0 (+inf: no bound)");
        if (ask_group >= MI_KNN_GROUPS_MAX && ask_group != MI_KNN_NO_GROUP)
            fail(MI_ERR_INVALID, "ask_group %u is neither a group id (< 2^24) nor MI_KNN_NO_GROUP", ask_group);
        if (voters) check_where(voters);
        check_table(t);
        std::lock_guard<std::mutex> l(t->mu);
        if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "a shard of a sharded table sees only its own voters");
        for (uint64_t& v : t->propose_stats) v = 0;
        const size_t rows = (size_t)t->rows;
        uint64_t tot[4] = {0, 0, 0, 0};
        auto no_proposals = [&] {
            std::fill(group, group + rows, MI_KNN_NO_GROUP);
            if (votes) std::fill(votes, votes + rows, 0u);
            if (heard) std::fill(heard, heard + rows, 0u);
            if (dist) std::fill(dist, dist + rows, INFINITY);
            if (totals) std::copy(tot, tot + 4, totals);
        };
        if (rows == 0) return no_proposals();
        SearchMany a;
        TableCall call(t);
        a.open(call);
        // who asks, who votes: two bitmaps and their counts, before any tile runs.  A voter holds a group, so a table without a
        // group column has none; a predicate nothing can meet leaves none either
        unsigned long long* d_clear = (unsigned long long*)a.scratch.get(2 * sizeof(unsigned long long));
        HIP_CHECK(hipMemsetAsync(d_clear, 0, 2 * sizeof(unsigned long long), a.s));
        a.row_mask = a.build_mask(every_live_row(), MASK_GROUP_IS, ask_group, d_clear);
        const bool can_vote = t->d_groups != nullptr && !(voters && where_never(*voters, true));
        if (can_vote) a.col_mask = a.build_mask(voters ? pred_of(*voters) : every_live_row(), MASK_GROUP_OTHER, ask_group, d_clear + 1);
        unsigned long long n[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(n, d_clear, sizeof n, hipMemcpyDeviceToHost, a.s));
        HIP_CHECK(hipStreamSynchronize(a.s));
        tot[0] = n[0]; tot[2] = n[1];
        if (n[0] == 0 || n[1] == 0) return no_proposals();
        a.matched = n[1];
        a.vote = true;
        a.hi_key = page_dist_key(max_dist);
        a.setup(call, (uint32_t)rows, k, false);
        uint64_t got[2] = {0, 0};
        a.run_vote(group, votes, heard, dist, got);
        tot[1] = got[0]; tot[3] = got[1];
        if (totals) std::copy(tot, tot + 4, totals);
    });
}

int mi_knn_propose_groups_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->propose_stats[i];
    });
}

int mi_knn_sharded_search_many(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, uint64_t* idx, float* dist) {
    return guarded([&] {
        ShardedCall call(t);
        check_args(t->shard[0], q, nq, k, idx, dist);
        // every shard on its own stream; the lists carry global ids and meet in mi_knn_merge's ordering, query by query
        ShardLists<> all(call.n, nq, k);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) { search_many_local(sh, q, nq, k, nullptr, all.idx(si), all.dist(si)); });
        merge_shard_lists(all, idx, dist);
    });
}

int mi_knn_sharded_search_many_where(mi_knn_sharded* t, const float* q, uint32_t nq, uint32_t k, const mi_knn_where* w, uint64_t* idx,
                                     float* dist, uint64_t* matched) {
    return guarded([&] {
        ShardedCall call(t);
        check_args(t->shard[0], q, nq, k, idx, dist);
        if (w) check_where(w);
        ShardLists<> all(call.n, nq, k, 1);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            all.counts(si)[0] = search_many_local(sh, q, nq, k, w, all.idx(si), all.dist(si));
        });
        merge_shard_lists(all, idx, dist);
        if (matched) all.sum_counts(matched);
    });
}

}  // extern "C"
