// join_between_walk.h — the walk over the column side of a join of two row sets, shared by the calls that consume it:
// the pair-emitting join (join_between.hip) and the density passes across shards (density_sharded.hip).
//
// Table A is the row side, on whose device and stream the work runs; table B, the column side, is a sequence of column chunks
// of whole tiles, each described by pointers that are valid on A's device: B's own mirror, rows and deletion bits when it
// lives there ("direct"), or a staged copy — the fp32 rows of chunk [c0, c1) copied into the call's scratch (device to
// device, or peer to peer from another GPU), mirrored there with knn_mirror_kernel, its deletion words built from B's host
// list.  Inside a chunk the rectangles a pair of bounds leaves (between_rects) are walked in strips of tile rows
// (tile_strips), halved after an overflow; what a strip does is the consumer's (rect_stages with its two stages).
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"
#include "handles.h"
#include "join_between_host.h"
#include "tile128.h"
#include "two_stage.h"

namespace mi {

// one column chunk as stage 1 and stage 2 see it: n rows that start at B's local row `off`; fn: the bound on its own rows
struct ColChunk {
    const uint16_t* mirror;
    const float* xx;
    const uint64_t* tomb;
    const float* rows;
    uint32_t n, off, fn;
};

// B in column chunks of whole tiles: what a staged chunk's scratch holds, and a block of columns whose mirror stays in the
// last-level cache while the row strips pass over it (a direct column side is cut the same way, by pointer).  a->mu and
// b->mu held, A's device selected, neither table empty; s = A's stream, which has been ordered behind B's pending work.
// have_b (nullable): B's mirror when the caller keeps one for the call (direct chunks read it instead of building one).
struct ColumnWalk {
    mi_knn *a, *b;
    hipStream_t s;
    bool staged;
    uint32_t chunk_rows, n_chunks;
    size_t words;
    TableMirror tb{nullptr, nullptr, nullptr};
    float* st_rows = nullptr;
    uint16_t* st_mirror = nullptr;
    float* st_xx = nullptr;
    uint64_t* st_tomb = nullptr;
    std::vector<uint64_t> h_tomb;

    ColumnWalk(mi_knn* a_, mi_knn* b_, hipStream_t s_, Scratch& scratch, const TableMirror* have_b = nullptr) : a(a_), b(b_), s(s_) {
        const uint64_t n_b = b->rows;
        staged = b->device != a->device || a->join_stage;
        chunk_rows = (uint32_t)std::min<uint64_t>(between_chunk_rows(a->dim, (uint32_t)a->join_stage_rows), (n_b + TILE - 1) / TILE * TILE);
        words = (chunk_rows + 63) / 64;
        if (!staged) {
            tb = have_b ? *have_b : table_mirror(b, s, scratch);
        } else {
            st_rows = (float*)scratch.get((size_t)chunk_rows * a->dim * sizeof(float));
            st_mirror = (uint16_t*)scratch.get((size_t)chunk_rows * a->dim * sizeof(uint16_t));
            st_xx = (float*)scratch.get((size_t)chunk_rows * sizeof(float));
            if (!b->dead.empty()) st_tomb = (uint64_t*)scratch.get(words * sizeof(uint64_t));
        }
        n_chunks = between_n_chunks(n_b, chunk_rows);
    }

    // Chunk ci as `col`, staged when it has to be; fn_b: the bound on B's local rows.  false: nothing of this chunk qualifies
    // under (fn_a of n_a rows, fn_b) and nothing was enqueued.  The caller waits for the stream before it asks for the next
    // chunk (staged: the scratch and h_tomb are then free again).
    bool chunk(uint32_t ci, uint32_t n_a, uint32_t fn_a, uint64_t fn_b, ColChunk* col) {
        uint64_t c0, c1;
        between_chunk(b->rows, chunk_rows, ci, &c0, &c1);
        const uint32_t cn = (uint32_t)(c1 - c0), cfn = between_chunk_bound(std::min<uint64_t>(fn_b, b->rows), c0, c1);
        if (fn_a >= n_a && cfn >= cn) return false;
        if (!staged) {
            // direct: B where it lies (c0 is a multiple of 128: whole deletion words)
            *col = ColChunk{tb.mirror + c0 * a->dim, tb.xx + c0, tb.tomb ? tb.tomb + c0 / 64 : nullptr, b->table + c0 * a->dim, cn,
                            (uint32_t)c0, cfn};
            return true;
        }
        // staged: the chunk's fp32 rows into this call's scratch on A's device, mirrored there
        const size_t bytes = (size_t)cn * a->dim * sizeof(float);
        const float* src = b->table + c0 * a->dim;
        if (b->device == a->device) HIP_CHECK(hipMemcpyAsync(st_rows, src, bytes, hipMemcpyDeviceToDevice, s));
        else HIP_CHECK(hipMemcpyPeerAsync(st_rows, a->device, src, b->device, bytes, s));
        mirror_rows(a, s, st_rows, 0, cn, st_mirror, st_xx);
        const uint64_t* tomb = nullptr;
        const auto d0 = std::lower_bound(b->dead.begin(), b->dead.end(), (uint32_t)c0);
        const auto d1 = std::lower_bound(d0, b->dead.end(), (uint32_t)std::min<uint64_t>(c1, 0xFFFFFFFFull));
        if (d0 != d1) {
            h_tomb.assign(words, 0ull);
            for (auto it = d0; it != d1; ++it) h_tomb[(*it - c0) >> 6] |= 1ull << ((*it - c0) & 63);
            HIP_CHECK(hipMemcpyAsync(st_tomb, h_tomb.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            tomb = st_tomb;
        }
        *col = ColChunk{st_mirror, st_xx, tomb, st_rows, cn, (uint32_t)c0, cfn};
        return true;
    }
};

// A chunk of n_b columns against all n_a rows of A: the rectangles (fn_a, fn_b) leave, in strips of tile rows.
// rect(br0, br1, bc0, bc1, &overflowed) runs one strip (rect_stages); stop() ends the walk between strips.
template <class Rect, class Stop>
void between_strips(uint32_t n_a, uint32_t n_b, uint32_t fn_a, uint32_t fn_b, Rect&& rect, Stop&& stop) {
    TileRect rects[2];
    const uint32_t n_rects = between_rects(n_a, n_b, fn_a, fn_b, rects);
    for (uint32_t i = 0; i < n_rects && !stop(); ++i)
        tile_strips(rects[i].r0, rects[i].r1, rects[i].c0, rects[i].c1, rect, stop);
}

}  // namespace mi
