// join_between.hip — host side of the threshold join of two row sets (mi_knn_near_pairs_between, mi_knn_sharded_near_pairs,
// mi_index_matches).  The kernels: join_between_kernels.h; the rules without HIP in them: join_between_host.h.
//
// One primitive (join_between) joins table A, the row side, on whose device and stream the work runs, with table B, the column
// side.  B is a sequence of column chunks, direct or staged, walked in strips of tile rows: join_between_walk.h, which the
// density passes across shards (density_sharded.hip) share.  The candidate buffer, the halving after an overflow (rect_stages)
// and the early stop behind user_cap are the self-join's (join.hip).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>

#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "handles.h"
#include "join_between_host.h"
#include "join_between_kernels.h"
#include "join_between_walk.h"
#include "sharded_call.h"
#include "two_stage.h"

using namespace mi;

static_assert(BETWEEN_TILE == (uint32_t)TILE, "join_between_host.h counts the tiles of tile128.h");

namespace {

struct Cross {
    mi_knn* a;
    hipStream_t s;
    const uint16_t* mirror_a;
    const float* xx_a;
    const uint64_t* tomb_a;
    uint32_t n_a, fn_a;
    ColChunk col;
    IdMap map_a, map_b;
    int by_id;
    float max_dist, c;
    uint32_t cand_cap;
    uint64_t user_cap;
    std::atomic<uint64_t>* total;   // pairs of the whole call so far (the sharded call: of every shard and shard pair)
    uint2 *d_cand, *d_pairs;
    float* d_dist;
    unsigned long long* d_count;   // [0]: candidates of the launch, [1] (low word): pairs stage 2 kept
    std::vector<uint2> h_pairs;
    std::vector<float> h_dist;
    std::vector<JoinPair> out;     // (A's local row, B's local row, distance)
    uint64_t stats[4] = {0, 0, 0, 0};
    bool over = false;

    // The stages for rect_stages (two_stage.h): every tile of the rectangle is computed; once more than user_cap pairs
    // qualify nothing more is launched (checked between launches: the call stops there).
    template <int NCH>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) -> unsigned long long {
            if (total->load() > user_cap) over = true;
            if (over) return 0;
            static DevOnce once;
            allow_lds_once(once, cross_tiles_kernel<NCH>, JOIN_LDS);
            HIP_CHECK(hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), s));
            hipLaunchKernelGGL((cross_tiles_kernel<NCH>), dim3(c1 - c0, r1 - r0), dim3(256), JOIN_LDS, s, mirror_a, xx_a, tomb_a, n_a,
                               col.mirror, col.xx, col.tomb, col.n, fn_a, col.fn, r0, c0, c, cand_cap, d_cand, d_count);
            HIP_CHECK(hipGetLastError());
            ++stats[2];
            stats[3] += (uint64_t)(r1 - r0) * (c1 - c0);
            return read_count(d_count, s);
        };
        auto stage2 = [&](uint32_t C) {
            stats[0] += C;
            hipLaunchKernelGGL((cross_rescore_kernel<NCH>), dim3(group16_blocks(a, C)), dim3(256), 0, s, a->table, col.rows, map_a, map_b,
                               col.off, by_id, d_cand, C, max_dist, d_pairs, d_dist, reinterpret_cast<uint32_t*>(d_count + 1));
            HIP_CHECK(hipGetLastError());
            uint32_t kept = 0;
            HIP_CHECK(hipMemcpyAsync(&kept, d_count + 1, sizeof kept, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (kept) {
                h_pairs.resize(kept);
                h_dist.resize(kept);
                HIP_CHECK(hipMemcpyAsync(h_pairs.data(), d_pairs, (size_t)kept * sizeof(uint2), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipMemcpyAsync(h_dist.data(), d_dist, (size_t)kept * sizeof(float), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                const size_t at = out.size();
                out.resize(at + kept);
                for (uint32_t j = 0; j < kept; ++j) out[at + j] = JoinPair{h_pairs[j].x, h_pairs[j].y, h_dist[j]};
            }
            stats[1] += kept;
            if (total->fetch_add(kept) + kept > user_cap) over = true;
        };
        rect_stages(br0, br1, bc0, bc1, cand_cap, overflowed, stage1, stage2);
    }

    // the chunk in `col` against all of A
    template <int NCH>
    void run_chunk() {
        between_strips(n_a, col.n, fn_a, col.fn,
                       [&](uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) { rect<NCH>(br0, br1, bc0, bc1, overflowed); },
                       [&] { return over; });
    }
};

// A (rows) x B (columns): the pairs of live rows within max_dist whose element passes (fn_a, fn_b) — local rows of A and B at or
// above which a row makes every pair of its own a candidate — as (A's local row, B's local row, distance), unordered.  by_id: the
// row with the smaller id is the query of a pair, else always A's.  total / user_cap: the early stop, *over = more than user_cap
// pairs qualify (out is then partial).  stats: {candidates, pairs, launches, tiles}, also left in a->between_stats.
void join_between(mi_knn* a, mi_knn* b, float max_dist, uint64_t fn_a, uint64_t fn_b, bool by_id, uint64_t user_cap,
                  std::atomic<uint64_t>* total, std::vector<JoinPair>* out, uint64_t stats[4], bool* over) {
    out->clear();
    *over = false;
    for (int i = 0; i < 4; ++i) stats[i] = 0;
    std::unique_lock<std::mutex> la(a->mu, std::defer_lock), lb(b->mu, std::defer_lock);
    std::lock(la, lb);   // (whichever order two concurrent calls name the tables in)
    for (uint64_t& v : a->between_stats) v = 0;
    if (a->dim != b->dim) fail(MI_ERR_INVALID, "the tables' dims differ (%u and %u)", a->dim, b->dim);
    check_mirror_dim(a->dim, "the join's");
    if (a->rows == 0 || b->rows == 0 || (fn_a >= a->rows && fn_b >= b->rows)) return;
    Scratch scratch;
    TableCall call(a);
    hipStream_t s = call.s;
    // behind B's pending writes (and the searches that share its mirror): their events, waited for on A's stream.  B's lock
    // is held until this call has waited for its own work, so nothing of B moves meanwhile.
    b->writes.begin(s);
    b->reads.begin(s);
    Cross j;
    j.a = a; j.s = s;
    j.n_a = (uint32_t)a->rows; j.fn_a = (uint32_t)std::min<uint64_t>(fn_a, a->rows);
    j.map_a = knn_id_map(a); j.map_b = knn_id_map(b);
    j.by_id = by_id ? 1 : 0;
    j.max_dist = max_dist;
    j.c = 1.0f - (max_dist + eps2(a->dim));
    j.cand_cap = std::max<uint32_t>(TILE_CAP_MIN, a->join_cap);
    j.user_cap = user_cap;
    j.total = total;
    const TableMirror tm = table_mirror(a, s, scratch);
    j.mirror_a = tm.mirror; j.xx_a = tm.xx; j.tomb_a = tm.tomb;
    j.d_cand = (uint2*)scratch.get((size_t)j.cand_cap * sizeof(uint2));
    j.d_pairs = (uint2*)scratch.get((size_t)j.cand_cap * sizeof(uint2));
    j.d_dist = (float*)scratch.get((size_t)j.cand_cap * sizeof(float));
    j.d_count = (unsigned long long*)scratch.get(2 * sizeof(unsigned long long));
    // B chunk by chunk (join_between_walk.h: direct or staged)
    ColumnWalk walk(a, b, s, scratch);
    for (uint32_t ci = 0; ci < walk.n_chunks && !j.over; ++ci) {
        if (!walk.chunk(ci, j.n_a, j.fn_a, fn_b, &j.col)) continue;   // nothing of this chunk qualifies
        dispatch_nch(a->dim, [&](auto nch) { j.template run_chunk<decltype(nch)::value>(); });
        HIP_CHECK(hipStreamSynchronize(s));   // (staged: the scratch and h_tomb are free for the next chunk)
    }
    for (int i = 0; i < 4; ++i) a->between_stats[i] = stats[i] = j.stats[i];
    *over = j.over;
    out->swap(j.out);
}

struct IdPair { uint64_t a, b; float d; };
void sort_pairs(std::vector<IdPair>* v) {
    std::sort(v->begin(), v->end(), [](const IdPair& x, const IdPair& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
}
[[noreturn]] void fail_over(uint64_t cap, float max_dist, uint64_t* count) {
    *count = cap + 1;
    fail(MI_ERR_UNSUPPORTED, "more than %llu pairs lie within %g: lower max_dist or raise cap", (unsigned long long)cap, (double)max_dist);
}

// mi_knn_near_pairs_between behind its argument check: A's row is the query, (id of t, id of other), ascending
void pairs_between(mi_knn* t, mi_knn* other, float max_dist, uint64_t cap, std::vector<IdPair>* res, bool* over) {
    std::vector<JoinPair> pairs;
    std::atomic<uint64_t> total{0};
    uint64_t stats[4];
    join_between(t, other, max_dist, 0, 0, false, cap, &total, &pairs, stats, over);
    res->clear();
    if (*over) return;
    // (the handles' id maps are fixed while they hold rows; ids ascend with the local rows on either side)
    const IdMap ma = knn_id_map(t), mb = knn_id_map(other);
    res->reserve(pairs.size());
    for (const JoinPair& p : pairs) res->push_back(IdPair{id_of_local(ma, p.a), id_of_local(mb, p.b), p.d});
    sort_pairs(res);
}

void write_pairs(const std::vector<IdPair>& res, uint64_t* a, uint64_t* b, float* dist, uint64_t* count) {
    for (size_t i = 0; i < res.size(); ++i) { a[i] = res[i].a; b[i] = res[i].b; dist[i] = res[i].d; }
    *count = res.size();
}

}  // namespace

extern "C" {

int mi_knn_near_pairs_between(mi_knn* t, mi_knn* other, float max_dist, uint64_t* a, uint64_t* b, float* dist, uint64_t cap,
                              uint64_t* count) {
    return guarded([&] {
        if (count) *count = 0;
        const char* why = "";
        const int bad = between_check_args(t, other, max_dist, a, b, dist, cap, count, &why);
        if (bad != MI_OK) fail(bad, "%s (max_dist %g, cap %llu)", why, (double)max_dist, (unsigned long long)cap);
        std::vector<IdPair> res;
        bool over = false;
        pairs_between(t, other, max_dist, cap, &res, &over);
        if (over) fail_over(cap, max_dist, count);
        write_pairs(res, a, b, dist, count);
    });
}

int mi_knn_near_pairs_between_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->between_stats[i];
    });
}

int mi_knn_sharded_near_pairs(mi_knn_sharded* t, float max_dist, uint64_t first_new, uint64_t* a, uint64_t* b, float* dist,
                              uint64_t cap, uint64_t* count) {
    return guarded([&] {
        if (count) *count = 0;
        const char* why = "";
        const int bad = sharded_join_check_args(t, max_dist, a, b, dist, cap, count, &why);
        if (bad != MI_OK) fail(bad, "%s (max_dist %g, cap %llu)", why, (double)max_dist, (unsigned long long)cap);
        ShardedCall call(t);
        if (first_new > t->rows)
            fail(MI_ERR_INVALID, "first_new %llu lies beyond one past the last row (%llu rows)", (unsigned long long)first_new,
                 (unsigned long long)t->rows);
        for (uint64_t& v : t->join_stats) v = 0;
        const uint32_t S = call.n;
        std::vector<uint64_t> fn(S);
        for (uint32_t si = 0; si < S; ++si) fn[si] = shard_first_new(t->block, S, si, first_new);
        std::atomic<uint64_t> total{0};
        std::vector<IdPair> res;
        std::mutex res_mu;
        bool over = false;
        // a piece's pairs (local rows of shards sa, sb) as global ids, the smaller first: what the one table reports
        auto take = [&](const std::vector<JoinPair>& pairs, mi_knn* sa, mi_knn* sb, const uint64_t stats[4], bool piece_over) {
            const IdMap ma = knn_id_map(sa), mb = knn_id_map(sb);
            std::lock_guard<std::mutex> lr(res_mu);
            for (int i = 0; i < 4; ++i) t->join_stats[i] += stats[i];
            over = over || piece_over;
            for (const JoinPair& p : pairs) {
                const uint64_t x = id_of_local(ma, p.a), y = id_of_local(mb, p.b);
                res.push_back(IdPair{std::min(x, y), std::max(x, y), p.d});
            }
        };
        // the S self-joins, side by side
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            std::vector<JoinPair> pairs;
            bool piece_over = false;
            knn_near_pairs_local(sh, max_dist, fn[si], cap, &pairs, &piece_over);
            uint64_t stats[4];
            {
                std::lock_guard<std::mutex> ls(sh->mu);
                for (int i = 0; i < 4; ++i) stats[i] = sh->join_stats[i];
            }
            total.fetch_add(pairs.size());
            take(pairs, sh, sh, stats, piece_over);
        });
        if (total.load() > cap) over = true;
        // the shard pairs, round by round: the pairs of a round share no shard, each on a host thread of its own
        for (const std::vector<ShardPair>& round : between_schedule(S)) {
            if (over) break;
            call.for_each_shard_pair(round, [&](uint32_t ra, uint32_t cb) {
                std::vector<JoinPair> pairs;
                bool piece_over = false;
                uint64_t stats[4];
                join_between(t->shard[ra], t->shard[cb], max_dist, fn[ra], fn[cb], true, cap, &total, &pairs, stats, &piece_over);
                take(pairs, t->shard[ra], t->shard[cb], stats, piece_over);
            });
        }
        if (over || res.size() > cap) fail_over(cap, max_dist, count);
        sort_pairs(&res);
        write_pairs(res, a, b, dist, count);
    });
}

int mi_knn_sharded_near_pairs_stats(mi_knn_sharded* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->join_stats[i];
    });
}

int mi_index_matches(mi_index* ix, mi_index* other, float max_dist, uint64_t* a, uint64_t* b, float* dist, uint64_t cap,
                     uint64_t* count) {
    return guarded([&] {
        if (count) *count = 0;
        const char* why = "";
        const int bad = between_check_args(ix, other, max_dist, a, b, dist, cap, count, &why);
        if (bad != MI_OK) fail(bad, "%s (max_dist %g, cap %llu)", why, (double)max_dist, (unsigned long long)cap);
        std::vector<IdPair> res;
        bool over = false;
        // (a removed path's rows are deleted rows of its table: the join never reports them)
        pairs_between(mi_index_table(ix), mi_index_table(other), max_dist, cap, &res, &over);
        if (over) fail_over(cap, max_dist, count);
        write_pairs(res, a, b, dist, count);
    });
}

}  // extern "C"
