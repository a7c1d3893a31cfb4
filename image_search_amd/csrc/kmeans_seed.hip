// kmeans_seed.hip — host side of mi_knn_kmeans_seed (k-means++ seeding over the live rows or a chosen subset, exact and
// deterministic).  The kernels and why the picks can be restated to the bit: kmeans_seed_kernels.h.
//
// One call: the candidates' local rows go up as a list, z_0 .. z_C (splitmix64) as an array, then 2 C + 2 launches are
// enqueued back to back — the first pass (usable rows), C x (pick, pass against the pick), the total — followed by the
// gather of the picked rows.  The host waits once.
#include <algorithm>
#include <cmath>

#include <mutex>
#include <vector>

#include "common.h"
#include "handles.h"
#include "kmeans_seed_kernels.h"
#include "two_stage.h"

using namespace mi;

namespace {

constexpr uint32_t SEED_MAX_C = 65536;

// the candidates' local rows, ascending, once each, deleted rows left out.  t->mu held, t->cyc_n <= 1.
std::vector<uint32_t> candidates(const mi_knn* t, const uint64_t* among, uint64_t n_among) {
    std::vector<uint32_t> rows;
    if (!among) {
        rows.reserve((size_t)(t->rows - t->dead.size()));
        size_t at = 0;
        for (uint64_t r = 0; r < t->rows; ++r) {
            if (at < t->dead.size() && t->dead[at] == r) { ++at; continue; }
            rows.push_back((uint32_t)r);
        }
        return rows;
    }
    rows.resize((size_t)n_among);
    for (uint64_t i = 0; i < n_among; ++i) {
        if (among[i] < t->base || among[i] - t->base >= t->rows)
            fail(MI_ERR_INVALID, "id %llu is not a row of this table (base %llu, %llu rows)", (unsigned long long)among[i],
                 (unsigned long long)t->base, (unsigned long long)t->rows);
        rows[i] = (uint32_t)(among[i] - t->base);
    }
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    std::vector<uint32_t> live(rows.size());
    live.resize((size_t)(std::set_difference(rows.begin(), rows.end(), t->dead.begin(), t->dead.end(), live.begin()) - live.begin()));
    return live;
}

}  // namespace

extern "C" {

int mi_knn_kmeans_seed(mi_knn* t, uint32_t C, uint64_t seed, const uint64_t* among, uint64_t n_among, uint64_t* rows, float* centroids,
                       double* potential) {
    return guarded([&] {
        if (potential) *potential = 0.0;
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        if (!rows) fail(MI_ERR_INVALID, "rows is null");
        if (C == 0) fail(MI_ERR_INVALID, "C must be >= 1");
        if (!among && n_among != 0) fail(MI_ERR_INVALID, "among is null");
        if (C > SEED_MAX_C) fail(MI_ERR_UNSUPPORTED, "at most %u seeds (got %u)", SEED_MAX_C, C);
        const uint32_t nch = t->dim / 64;
        if (t->dim % 64 != 0 || (nch != 2 && nch != 4 && nch != 8 && nch != 12 && nch != 16))
            fail(MI_ERR_UNSUPPORTED, "dim %u: the seeding is built for dim in {128, 256, 512, 768, 1024}", t->dim);
        if (t->rows > 0xFFFFFFFFull) fail(MI_ERR_UNSUPPORTED, "a shard holds at most 2^32-1 rows");
        std::lock_guard<std::mutex> l(t->mu);
        for (uint64_t& v : t->kmeans_seed_stats) v = 0;
        if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "not offered on a shard of a sharded table");
        const std::vector<uint32_t> list = candidates(t, among, n_among);   // every id checked before anything runs
        const uint32_t S = (uint32_t)list.size();
        if (C > S) fail(MI_ERR_INVALID, "%u seeds from %u candidate rows", C, S);

        std::vector<unsigned long long> z((size_t)C + 1);   // splitmix64 started at `seed`
        uint64_t state = seed;
        for (unsigned long long& out : z) {
            state += 0x9E3779B97F4A7C15ull;
            uint64_t v = state;
            v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
            v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
            out = v ^ (v >> 31);
        }

        std::vector<uint32_t> picks(C);
        uint32_t h_state[2] = {0, 0};
        unsigned long long total = 0;
        Scratch scratch;
        TableCall call(t);
        hipStream_t s = call.s;
        // a chunk: as many positions as keep the chunk sums within what one pick scans
        const uint32_t per = (uint32_t)(((uint64_t)S + (uint64_t)KMPP_CHUNK * KMPP_MAX_CHUNKS - 1) / ((uint64_t)KMPP_CHUNK * KMPP_MAX_CHUNKS));
        const uint32_t chunk = KMPP_CHUNK * std::max(1u, per);
        const uint32_t n_chunks = (uint32_t)(((uint64_t)S + chunk - 1) / chunk);
        uint32_t* d_list = (uint32_t*)scratch.get((size_t)S * sizeof(uint32_t));
        float* d_D = (float*)scratch.get((size_t)S * sizeof(float));
        uint32_t* d_w = (uint32_t*)scratch.get((size_t)S * sizeof(uint32_t));
        uint32_t* d_flags = (uint32_t*)scratch.get((size_t)S * sizeof(uint32_t));
        unsigned long long* d_sum = (unsigned long long*)scratch.get((size_t)n_chunks * sizeof(unsigned long long));
        unsigned long long* d_z = (unsigned long long*)scratch.get(z.size() * sizeof(unsigned long long));
        unsigned long long* d_total = (unsigned long long*)scratch.get(sizeof(unsigned long long));
        uint32_t* d_picks = (uint32_t*)scratch.get((size_t)C * sizeof(uint32_t));
        uint32_t* d_state = (uint32_t*)scratch.get(2 * sizeof(uint32_t));
        float* d_cent = centroids ? (float*)scratch.get((size_t)C * t->dim * sizeof(float)) : nullptr;
        HIP_CHECK(hipMemcpyAsync(d_list, list.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_z, z.data(), z.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_picks, 0, (size_t)C * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(d_state, 0, 2 * sizeof(uint32_t), s));

        dispatch_nch(t->dim, [&](auto nch_c) {
            constexpr int NCH = decltype(nch_c)::value;
            hipLaunchKernelGGL((kmpp_pass_kernel<NCH, true>), dim3(n_chunks), dim3(256), 0, s, t->table, d_list, S, chunk,
                               (const uint32_t*)nullptr, d_D, d_w, d_flags, d_sum);
            for (uint32_t j = 0; j < C; ++j) {
                hipLaunchKernelGGL(kmpp_pick_kernel, dim3(1), dim3(1024), 0, s, d_sum, n_chunks, chunk, S, d_w, d_flags, d_z, j, C, d_picks,
                                   d_state, d_total);
                hipLaunchKernelGGL((kmpp_pass_kernel<NCH, false>), dim3(n_chunks), dim3(256), 0, s, t->table, d_list, S, chunk,
                                   d_picks + j, d_D, d_w, d_flags, d_sum);
            }
            hipLaunchKernelGGL(kmpp_pick_kernel, dim3(1), dim3(1024), 0, s, d_sum, n_chunks, chunk, S, d_w, d_flags, d_z, C, C, d_picks, d_state,
                               d_total);
        });
        HIP_CHECK(hipGetLastError());
        if (centroids) {
            hipLaunchKernelGGL(kmpp_gather_kernel, dim3(C), dim3(256), 0, s, t->table, d_list, d_picks, t->dim, d_cent);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemcpyAsync(picks.data(), d_picks, (size_t)C * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_state, d_state, sizeof h_state, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, s));
        if (centroids) HIP_CHECK(hipMemcpyAsync(centroids, d_cent, (size_t)C * t->dim * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (uint32_t j = 0; j < C; ++j) {
            if (picks[j] >= S) fail(MI_ERR_HIP, "pick %u came back as position %u of %u", j, picks[j], S);
            rows[j] = t->base + list[picks[j]];
        }
        if (potential) *potential = std::ldexp((double)total, -30);
        t->kmeans_seed_stats[0] = S;
        t->kmeans_seed_stats[1] = (uint64_t)C + 1;
        t->kmeans_seed_stats[2] = h_state[1];
    });
}

int mi_knn_kmeans_seed_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->kmeans_seed_stats[i];
    });
}

}  // extern "C"
