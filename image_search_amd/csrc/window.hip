// window.hip — the windowed stage 1 of mi_knn_near_pairs_window, mi_knn_density_window and mi_knn_dbscan_window (the calls
// themselves stand beside their unwindowed siblings in join.hip and density.hip), and mi_knn_window_stats.  The kernels:
// window_kernels.h; the host-only rules (the gap, the columns a strip launches, the tile counts): window_host.h.
#include <mutex>

#include "common.h"
#include "handles.h"
#include "two_stage.h"
#include "window_call.h"
#include "window_kernels.h"

namespace mi {

void window_ranges(mi_knn* t, hipStream_t s, Scratch& scratch, uint64_t window, WindowCall* w) {
    const uint32_t n_rows = (uint32_t)t->rows, n_blocks = (n_rows + TILE - 1) / TILE;
    StampRange* d_range = (StampRange*)scratch.get((size_t)n_blocks * sizeof(StampRange));
    const uint64_t* tomb = t->dead.empty() ? nullptr : t->d_tomb;
    hipLaunchKernelGGL(stamp_ranges_kernel, dim3(n_blocks), dim3(TILE), 0, s, t->d_stamps, tomb, n_rows, d_range);
    HIP_CHECK(hipGetLastError());
    // the ranges, read back once: the host decides from them what the tiles of both passes do
    read_back(&w->blocks.range, d_range, n_blocks, s);
    HIP_CHECK(hipStreamSynchronize(s));
    w->blocks.window = window;
    w->win = PairWindow{t->d_stamps, d_range, window};
}

namespace {

template <int NCH, int PASS>
void launch_tiles(WindowCall& w, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
    const dim3 grid(c1 - c0, r1 - r0);
    static DevOnce once;   // one per kernel
    if constexpr (PASS == 1) {
        allow_lds_once(once, window_tiles_kernel<NCH>, WINDOW_LDS);
        hipLaunchKernelGGL((window_tiles_kernel<NCH>), grid, dim3(256), WINDOW_LDS, w.s, w.mirror, w.xx, w.tomb, w.n_rows, w.first_new, r0,
                           c0, w.c, w.cand_cap, w.d_cand, w.d_count, w.win);
    } else {
        allow_lds_once(once, window_skip_tiles_kernel<NCH>, WINDOW_LDS);
        hipLaunchKernelGGL((window_skip_tiles_kernel<NCH>), grid, dim3(256), WINDOW_LDS, w.s, w.mirror, w.xx, w.tomb, w.d_act, w.n_rows, r0,
                           c0, w.c, w.cand_cap, w.d_cand, w.d_count, w.win);
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace

unsigned long long window_stage1(WindowCall& w, int pass, uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) {
    c0 = std::max(c0, r0);
    if (c0 >= c1) return 0;
    const int tiles = pass == 1 ? WS_TILES1 : WS_TILES2, skipped = pass == 1 ? WS_SKIPPED1 : WS_SKIPPED2;
    const WindowStrip strip = window_strip(w.blocks, r0, r1, c0, c1);
    if (!strip.launches()) { w.stats[skipped] += strip.skipped; return 0; }   // every workgroup would leave at once
    HIP_CHECK(hipMemsetAsync(w.d_count, 0, w.count_words * sizeof(unsigned long long), w.s));
    dispatch_nch(w.dim, [&](auto nch) {
        if (pass == 1) launch_tiles<decltype(nch)::value, 1>(w, r0, r1, strip.lo, strip.hi);
        else launch_tiles<decltype(nch)::value, 2>(w, r0, r1, strip.lo, strip.hi);
    });
    ++w.stats[WS_LAUNCHES];
    const unsigned long long n = read_count(w.d_count, w.s);
    if (n <= w.cand_cap) { w.stats[tiles] += strip.computed; w.stats[skipped] += strip.skipped; }
    return n;
}

}  // namespace mi

extern "C" int mi_knn_window_stats(mi_knn* t, uint64_t out[8]) {
    return mi::guarded([&] {
        if (!t || !out) mi::fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 8; ++i) out[i] = t->window_stats[i];
    });
}
