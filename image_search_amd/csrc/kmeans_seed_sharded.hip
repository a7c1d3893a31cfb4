// kmeans_seed_sharded.hip — host side of mi_knn_sharded_kmeans_seed and mi_knn_sharded_kmeans_seed_stats: the k-means++
// seeding of mi_knn_kmeans_seed over a block-cyclic table, bit for bit what one table holding the same rows returns.  The
// plan (candidates per shard, chunks, the global order, the bytes exchanged): kmeans_seed_sharded_host.h; the kernels:
// kmeans_seed_sharded_kernels.h.
//
// Streams: a shard's work runs on its own stream.  Per seed the first shard's stream waits for the event behind every other
// shard's pass (then copies its chunk sums) and behind its locate (then copies its slot); every other shard's stream waits
// for the event behind the pick (then copies the pick word) and behind the select (then copies the centre).  Everything is
// enqueued; the host waits once at the end.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "kmeans_seed_sharded_host.h"
#include "kmeans_seed_sharded_kernels.h"
#include "sharded_call.h"
#include "two_stage.h"

using namespace mi;

namespace {

constexpr uint32_t SEED_MAX_C = 65536;

// one shard's state for the call; its device memory lives in `scratch`, on the shard's device
struct SeedShard {
    Scratch scratch;
    mi_knn* sh = nullptr;
    hipStream_t s = nullptr;
    Event ev;                             // shard >= 1: its words / its slot are in place; shard 0: the pick word / the centre is
    IdMap map{0, 0, 0, 0};
    uint32_t n_list = 0, n_chunks = 0;
    uint32_t* d_list = nullptr;
    KmppChunk* d_desc = nullptr;
    float* d_D = nullptr;
    uint32_t *d_w = nullptr, *d_flags = nullptr, *d_cursor = nullptr;
    unsigned long long* d_words = nullptr;   // [1 + n_chunks]: the lowest unpicked global id, then the chunk sums
    unsigned long long* d_slot = nullptr;    // [kmpp_slot_words]
    KmppPick* d_pick = nullptr;
    float* d_centre = nullptr;               // [dim]
};

// every shard's stream idle before the call's device memory goes, and its order word saying so (what TableCall leaves
// behind, scan_call.h), on every way out
struct Drain {
    std::vector<std::unique_ptr<SeedShard>>& st;
    ~Drain() {
        for (auto& x : st)
            if (x && x->s) {
                std::lock_guard<std::mutex> l(x->sh->mu);
                (void)hipStreamSynchronize(x->s);
                x->sh->reads.pending = false;
            }
    }
};

// the live candidates as global ids, ascending, once each; every id was checked by the frame's router.  t->mu held
std::vector<uint64_t> candidates(mi_knn_sharded* t, const uint64_t* among, uint64_t n_among) {
    std::vector<uint64_t> ids;
    if (among) {
        ids.assign(among, among + n_among);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    } else {
        ids.resize((size_t)t->rows);
        for (uint64_t r = 0; r < t->rows; ++r) ids[(size_t)r] = r;
    }
    const std::vector<uint64_t> dead = sharded_deleted(t);   // ascending
    if (dead.empty()) return ids;
    std::vector<uint64_t> live(ids.size());
    live.resize((size_t)(std::set_difference(ids.begin(), ids.end(), dead.begin(), dead.end(), live.begin()) - live.begin()));
    return live;
}

template <int NCH, bool FIRST>
void launch_pass(SeedShard& x) {
    if (x.n_chunks == 0) return;   // a shard without candidates takes part with its lowest-unpicked word alone
    hipLaunchKernelGGL((kmpp_sharded_pass_kernel<NCH, FIRST>), dim3(x.n_chunks), dim3(256), 0, x.s, x.sh->table, x.d_list, x.d_desc,
                       x.d_centre, x.d_D, x.d_w, x.d_flags, x.d_words + 1);
    HIP_CHECK(hipGetLastError());
}

struct SeedOut {
    std::vector<uint64_t> rows;
    std::vector<float> centroids;
    unsigned long long total = 0;
    uint32_t fallbacks = 0;
};

// arguments checked; the plan made; everything lands in `out`
void sharded_seed_run(ShardedCall& call, const KmppPlan& plan, uint32_t C, uint64_t seed, bool want_centroids, SeedOut* out) {
    mi_knn_sharded* t = call.t;
    const uint32_t S = call.n, dim = t->dim, G = (uint32_t)plan.order.size();
    const uint32_t slot_words = kmpp_slot_words(dim);
    const size_t slot_bytes = (size_t)slot_words * sizeof(unsigned long long);

    std::vector<unsigned long long> z((size_t)C + 1);   // splitmix64 started at `seed`
    uint64_t state = seed;
    for (unsigned long long& o : z) {
        state += 0x9E3779B97F4A7C15ull;
        uint64_t v = state;
        v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
        v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
        o = v ^ (v >> 31);
    }

    // where every shard's words lie on the first shard's device, and the global order as indices into them
    std::vector<uint32_t> low_at(S), sum_at(G);
    uint64_t n_words = 0;
    for (uint32_t si = 0; si < S; ++si) {
        low_at[si] = (uint32_t)n_words;
        n_words += 1 + plan.shard[si].chunks.size();
    }
    if (n_words > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "%llu chunk words", (unsigned long long)n_words);
    for (uint32_t g = 0; g < G; ++g) sum_at[g] = low_at[plan.order[g].shard] + 1 + plan.order[g].chunk;

    std::vector<std::unique_ptr<SeedShard>> st(S);
    for (uint32_t si = 0; si < S; ++si) st[si].reset(new SeedShard);
    Drain drain{st};

    // the first shard's side of the exchange
    unsigned long long *d_all = nullptr, *d_slots = nullptr, *d_z = nullptr, *d_rows = nullptr, *d_total = nullptr;
    uint32_t *d_low_at = nullptr, *d_sum_at = nullptr, *d_fallbacks = nullptr;
    KmppChunkAt* d_order = nullptr;
    float* d_cent = nullptr;

    // the shards' state.  (Not a TableCall: it would wait for the stream where it closes; the stream is ordered behind the
    // shard's earlier work by hand and settled with the results.)
    for (uint32_t si = 0; si < S; ++si) {
        mi_knn* sh = t->shard[si];
        std::lock_guard<std::mutex> l(sh->mu);
        DeviceGuard g(sh->device);
        SeedShard& x = *st[si];
        const KmppShardPlan& mine = plan.shard[si];
        x.sh = sh;
        x.map = knn_id_map(sh);
        x.n_list = (uint32_t)mine.rows.size();
        x.n_chunks = (uint32_t)mine.chunks.size();
        x.s = knn_own_stream(sh);
        sh->writes.begin(x.s);
        sh->reads.begin(x.s);
        x.ev.get(hipEventDisableTiming);
        if (si == 0) {
            d_all = (unsigned long long*)x.scratch.get((size_t)n_words * sizeof(unsigned long long));
            d_slots = (unsigned long long*)x.scratch.get((size_t)S * slot_bytes);
            d_z = (unsigned long long*)x.scratch.get(z.size() * sizeof(unsigned long long));
            d_rows = (unsigned long long*)x.scratch.get((size_t)C * sizeof(unsigned long long));
            d_total = (unsigned long long*)x.scratch.get(sizeof(unsigned long long));
            d_low_at = (uint32_t*)x.scratch.get((size_t)S * sizeof(uint32_t));
            d_sum_at = (uint32_t*)x.scratch.get((size_t)G * sizeof(uint32_t));
            d_order = (KmppChunkAt*)x.scratch.get((size_t)G * sizeof(KmppChunkAt));
            d_fallbacks = (uint32_t*)x.scratch.get(sizeof(uint32_t));
            if (want_centroids) d_cent = (float*)x.scratch.get((size_t)C * dim * sizeof(float));
            HIP_CHECK(hipMemcpyAsync(d_z, z.data(), z.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, x.s));
            HIP_CHECK(hipMemcpyAsync(d_low_at, low_at.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, x.s));
            HIP_CHECK(hipMemcpyAsync(d_sum_at, sum_at.data(), (size_t)G * sizeof(uint32_t), hipMemcpyHostToDevice, x.s));
            HIP_CHECK(hipMemcpyAsync(d_order, plan.order.data(), (size_t)G * sizeof(KmppChunkAt), hipMemcpyHostToDevice, x.s));
            HIP_CHECK(hipMemsetAsync(d_rows, 0xFF, (size_t)C * sizeof(unsigned long long), x.s));
            HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(unsigned long long), x.s));
            HIP_CHECK(hipMemsetAsync(d_fallbacks, 0, sizeof(uint32_t), x.s));
            // the first shard's words and slot are written where the pick and the select read them
            x.d_words = d_all + low_at[0];
            x.d_slot = d_slots;
        } else {
            x.d_words = (unsigned long long*)x.scratch.get((size_t)(1 + x.n_chunks) * sizeof(unsigned long long));
            x.d_slot = (unsigned long long*)x.scratch.get(slot_bytes);
        }
        x.d_list = (uint32_t*)x.scratch.get((size_t)x.n_list * sizeof(uint32_t));
        x.d_desc = (KmppChunk*)x.scratch.get((size_t)x.n_chunks * sizeof(KmppChunk));
        x.d_D = (float*)x.scratch.get((size_t)x.n_list * sizeof(float));
        x.d_w = (uint32_t*)x.scratch.get((size_t)x.n_list * sizeof(uint32_t));
        x.d_flags = (uint32_t*)x.scratch.get((size_t)x.n_list * sizeof(uint32_t));
        x.d_cursor = (uint32_t*)x.scratch.get(sizeof(uint32_t));
        x.d_pick = (KmppPick*)x.scratch.get(sizeof(KmppPick));
        x.d_centre = (float*)x.scratch.get((size_t)dim * sizeof(float));
        if (x.n_list != 0) {
            HIP_CHECK(hipMemcpyAsync(x.d_list, mine.rows.data(), (size_t)x.n_list * sizeof(uint32_t), hipMemcpyHostToDevice, x.s));
            HIP_CHECK(hipMemcpyAsync(x.d_desc, mine.chunks.data(), (size_t)x.n_chunks * sizeof(KmppChunk), hipMemcpyHostToDevice, x.s));
        }
        // nothing is picked yet: the lowest unpicked id is the first candidate's
        const unsigned long long low0 = x.n_list != 0 ? id_of_local(x.map, mine.rows[0]) : ~0ull;
        HIP_CHECK(hipMemcpyAsync(x.d_words, &low0, sizeof low0, hipMemcpyHostToDevice, x.s));
        HIP_CHECK(hipMemsetAsync(x.d_cursor, 0, sizeof(uint32_t), x.s));
        HIP_CHECK(hipMemsetAsync(x.d_slot, 0, slot_bytes, x.s));
        HIP_CHECK(hipStreamSynchronize(x.s));   // (low0 and the plan's vectors are pageable host memory)
    }

    // f(si, shard state) with the shard's lock held and its device selected
    auto on_shard = [&](uint32_t si, auto&& f) {
        SeedShard& x = *st[si];
        std::lock_guard<std::mutex> l(x.sh->mu);
        DeviceGuard g(x.sh->device);
        f(x);
    };
    SeedShard& zs = *st[0];
    // every shard's words to the first shard, then pick j there (j == C: the total alone)
    auto gather_and_pick = [&](uint32_t j) {
        for (uint32_t si = 1; si < S; ++si) on_shard(si, [&](SeedShard& x) { HIP_CHECK(hipEventRecord(x.ev, x.s)); });
        on_shard(0, [&](SeedShard& x) {
            for (uint32_t si = 1; si < S; ++si) {
                SeedShard& y = *st[si];
                HIP_CHECK(hipStreamWaitEvent(x.s, y.ev, 0));
                copy_between(d_all + low_at[si], x.sh->device, y.d_words, y.sh->device, (size_t)(1 + y.n_chunks) * sizeof(unsigned long long),
                             x.s);
            }
            hipLaunchKernelGGL(kmpp_sharded_pick_kernel, dim3(1), dim3(1024), 0, x.s, (const unsigned long long*)d_all,
                               (const uint32_t*)d_low_at, S, (const uint32_t*)d_sum_at, (const KmppChunkAt*)d_order, G,
                               (const unsigned long long*)d_z, j, C, x.d_pick, d_fallbacks, d_total);
            HIP_CHECK(hipGetLastError());
            if (j < C) HIP_CHECK(hipEventRecord(x.ev, x.s));
        });
    };

    dispatch_nch(dim, [&](auto nch_c) {
        constexpr int NCH = decltype(nch_c)::value;
        for (uint32_t si = 0; si < S; ++si) on_shard(si, [&](SeedShard& x) { launch_pass<NCH, true>(x); });
        for (uint32_t j = 0; j < C; ++j) {
            gather_and_pick(j);
            // the pick word to every shard; the owner finds the row
            for (uint32_t si = 0; si < S; ++si)
                on_shard(si, [&](SeedShard& x) {
                    if (si != 0) {
                        HIP_CHECK(hipStreamWaitEvent(x.s, zs.ev, 0));
                        copy_between(x.d_pick, x.sh->device, zs.d_pick, zs.sh->device, sizeof(KmppPick), x.s);
                    }
                    hipLaunchKernelGGL(kmpp_sharded_locate_kernel, dim3(1), dim3(256), 0, x.s, (const float*)x.sh->table,
                                       (const uint32_t*)x.d_list, x.n_list, (const KmppChunk*)x.d_desc, x.n_chunks, (const KmppPick*)x.d_pick, si,
                                       x.map, dim, x.d_w, x.d_flags, x.d_cursor, x.d_words, x.d_slot);
                    HIP_CHECK(hipGetLastError());
                    if (si != 0) HIP_CHECK(hipEventRecord(x.ev, x.s));
                });
            // the slots to the first shard; the flagged one is seed j and the next centre
            on_shard(0, [&](SeedShard& x) {
                for (uint32_t si = 1; si < S; ++si) {
                    SeedShard& y = *st[si];
                    HIP_CHECK(hipStreamWaitEvent(x.s, y.ev, 0));
                    copy_between(d_slots + (size_t)si * slot_words, x.sh->device, y.d_slot, y.sh->device, slot_bytes, x.s);
                }
                hipLaunchKernelGGL(kmpp_sharded_select_kernel, dim3(1), dim3(256), 0, x.s, (const unsigned long long*)d_slots, slot_words, S,
                                   dim, j, d_rows, d_cent, x.d_centre);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipEventRecord(x.ev, x.s));
            });
            // the centre to every shard; the pass against it
            for (uint32_t si = 0; si < S; ++si)
                on_shard(si, [&](SeedShard& x) {
                    if (si != 0) {
                        HIP_CHECK(hipStreamWaitEvent(x.s, zs.ev, 0));
                        copy_between(x.d_centre, x.sh->device, zs.d_centre, zs.sh->device, (size_t)dim * sizeof(float), x.s);
                    }
                    launch_pass<NCH, false>(x);
                });
        }
        gather_and_pick(C);
    });

    // one wait: the ids, the centroids, the total and the fallback count from the first shard
    SeedOut res;
    res.rows.resize(C);
    if (want_centroids) res.centroids.resize((size_t)C * dim);
    on_shard(0, [&](SeedShard& x) {
        HIP_CHECK(hipMemcpyAsync(res.rows.data(), d_rows, (size_t)C * sizeof(unsigned long long), hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipMemcpyAsync(&res.total, d_total, sizeof res.total, hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipMemcpyAsync(&res.fallbacks, d_fallbacks, sizeof res.fallbacks, hipMemcpyDeviceToHost, x.s));
        if (want_centroids)
            HIP_CHECK(hipMemcpyAsync(res.centroids.data(), d_cent, (size_t)C * dim * sizeof(float), hipMemcpyDeviceToHost, x.s));
        HIP_CHECK(hipStreamSynchronize(x.s));
    });
    for (uint32_t si = 1; si < S; ++si) on_shard(si, [&](SeedShard& x) { HIP_CHECK(hipStreamSynchronize(x.s)); });
    for (uint32_t j = 0; j < C; ++j)
        if (res.rows[j] >= t->rows) fail(MI_ERR_HIP, "pick %u came back as id %llu of %llu rows", j, (unsigned long long)res.rows[j],
                                         (unsigned long long)t->rows);
    *out = std::move(res);
}

}  // namespace

extern "C" {

int mi_knn_sharded_kmeans_seed(mi_knn_sharded* t, uint32_t C, uint64_t seed, const uint64_t* among, uint64_t n_among, uint64_t* rows,
                               float* centroids, double* potential) {
    return guarded([&] {
        // (mi_knn_kmeans_seed's rules, in front of anything that follows the handle)
        if (potential) *potential = 0.0;
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (!rows) fail(MI_ERR_INVALID, "rows is null");
        if (C == 0) fail(MI_ERR_INVALID, "C must be >= 1");
        if (!among && n_among != 0) fail(MI_ERR_INVALID, "among is null");
        if (C > SEED_MAX_C) fail(MI_ERR_UNSUPPORTED, "at most %u seeds (got %u)", SEED_MAX_C, C);
        SeedOut out;
        {
            ShardedCall call(t);
            const uint32_t nch = t->dim / 64;
            if (t->dim % 64 != 0 || (nch != 2 && nch != 4 && nch != 8 && nch != 12 && nch != 16))
                fail(MI_ERR_UNSUPPORTED, "dim %u: the seeding is built for dim in {128, 256, 512, 768, 1024}", t->dim);
            if (t->rows > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)t->rows);
            for (uint64_t& v : t->kmeans_seed_stats) v = 0;
            call.route(among, n_among);   // every id checked before anything runs
            call.ready();
            const std::vector<uint64_t> ids = candidates(t, among, n_among);
            if (C > ids.size()) fail(MI_ERR_INVALID, "%u seeds from %llu candidate rows", C, (unsigned long long)ids.size());
            const KmppPlan plan = kmpp_sharded_plan(t->block, call.n, ids);
            sharded_seed_run(call, plan, C, seed, centroids != nullptr, &out);
            uint64_t elsewhere = 0;
            for (uint32_t si = 1; si < call.n; ++si) elsewhere += plan.shard[si].chunks.size();
            t->kmeans_seed_stats[0] = ids.size();
            t->kmeans_seed_stats[1] = (uint64_t)C + 1;
            t->kmeans_seed_stats[2] = out.fallbacks;
            t->kmeans_seed_stats[3] = kmpp_sharded_exchange_bytes(call.n, elsewhere, C, t->dim);
        }
        std::memcpy(rows, out.rows.data(), (size_t)C * sizeof(uint64_t));
        if (centroids) std::memcpy(centroids, out.centroids.data(), out.centroids.size() * sizeof(float));
        if (potential) *potential = std::ldexp((double)out.total, -30);
    });
}

int mi_knn_sharded_kmeans_seed_stats(mi_knn_sharded* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->kmeans_seed_stats[i];
    });
}

}  // extern "C"
