// window_call.h — what join.hip and density.hip need of the windowed stage 1 (window.hip, window_kernels.h): the calls
// mi_knn_near_pairs_window, mi_knn_density_window and mi_knn_dbscan_window are their unwindowed siblings with this stage 1 in
// place of join_tiles_kernel / density_tiles_kernel; everything behind it (stage 2, the strip walk, the overflow halving, the
// outputs) is the sibling's own code.
#pragma once
#include <cstdint>

#include "common.h"
#include "handles.h"
#include "pair_kernels.h"
#include "two_stage.h"
#include "window_host.h"

namespace mi {

// the eight words of mi_knn_window_stats
enum { WS_CAND1 = 0, WS_WITHIN, WS_TILES1, WS_SKIPPED1, WS_CAND2, WS_TILES2, WS_SKIPPED2, WS_LAUNCHES, WS_WORDS };

// one windowed call on a table: the operands of the self tiles, the window on the device and the blocks on the host
struct WindowCall {
    hipStream_t s = nullptr;
    uint32_t dim = 0, n_rows = 0, first_new = 0;   // first_new: a local row (the join's; the density passes: 0)
    const uint16_t* mirror = nullptr;
    const float* xx = nullptr;
    const uint64_t* tomb = nullptr;
    const uint8_t* d_act = nullptr;                // pass 2: the blocks' activity bytes on the device
    float c = 0.0f;                                // 1 - (max_dist + eps2)
    uint32_t cand_cap = 0;
    uint2* d_cand = nullptr;
    unsigned long long* d_count = nullptr;         // the word the launch in flight counts its candidates in
    uint32_t count_words = 1;                      // words zeroed in front of a launch (the join: 2, its stage 2 counts in the next)
    PairWindow win = {nullptr, nullptr, 0};
    WindowBlocks blocks;                           // the ranges, read back once; act: filled by the caller before pass 2
    uint64_t stats[WS_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};   // the tile and launch words; the caller adds candidates and pairs
};

// The block stamp ranges of t (stamp_ranges_kernel) into `scratch`, read back into w->blocks; sets w->win.  t->mu held, the
// device selected, t not empty.
void window_ranges(mi_knn* t, hipStream_t s, Scratch& scratch, uint64_t window, WindowCall* w);
// Stage 1 of pass `pass` (1 or 2) for rect_stages on the tile rows [r0, r1) x columns [c0, c1): c0 is raised to the diagonal,
// the launch covers only the columns where a tile survives the stamp ranges (pass 2: and the activity bytes), and none at all
// when no tile does.  Returns the candidates counted.  A launch whose candidates fit the buffer counts its tiles, as
// DensityStage1 does: computed + skipped = the ground, also across overflow halvings.
unsigned long long window_stage1(WindowCall& w, int pass, uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1);

}  // namespace mi
