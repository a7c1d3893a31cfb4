// density_sharded.hip — host side of mi_knn_sharded_density, mi_knn_sharded_dbscan and mi_knn_sharded_dbscan_stats: the
// density passes of density.hip over a block-cyclic table, the pairs that cross shards included.  The kernels and why every
// merge is order-free: density_sharded_kernels.h; the rules without HIP in them: density_sharded_host.h; the walk over a
// column shard's chunks, shared with the join: join_between_walk.h.
//
// Per shard, on its device, for the call: deg [local rows], bkey [local rows], activity bytes [local blocks] and a forest
// parent [G] over the GLOBAL rows of the table (4 bytes per table row per shard).  Pass 1 and pass 2 each run the S self
// pieces side by side and then the shard pairs in between_schedule's rounds (no shard twice in a round: the column shard of a
// pair is idle, so the row side's stream may add into its arrays, or the host may merge a staged chunk's arrays into them).
// Then forest s = 1 .. S - 1 is copied to shard 0's device and united into forest 0, the roots go back to every shard, and
// every shard resolves its local rows; the host scatters them to global rows.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "density_call.h"
#include "density_sharded_host.h"
#include "density_sharded_kernels.h"
#include "handles.h"
#include "join_between_walk.h"
#include "sharded_call.h"
#include "two_stage.h"

using namespace mi;

namespace mi {

// ---- the small kernels between the pieces --------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void density_forest_init_kernel(uint32_t* __restrict__ parent, uint32_t n) {
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n; g += gridDim.x * 256) parent[g] = g;
}
// a staged chunk's degrees / border keys into the column shard's own, on its device (the shard is idle meanwhile)
static __global__ __launch_bounds__(256) void density_add_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t n) {
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) dst[r] += src[r];
}
static __global__ __launch_bounds__(256) void density_min_kernel(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ src,
                                                          uint32_t n) {
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) dst[r] = min(dst[r], src[r]);
}

// other[i] = the parent of global row g0 + i in another shard's forest, copied here: where that is no root, a union in `parent`
static __global__ __launch_bounds__(256) void density_forest_merge_kernel(uint32_t* parent, const uint32_t* __restrict__ other, uint32_t g0,
                                                                   uint32_t n, unsigned long long* __restrict__ words) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t g = g0 + i, p = other[i];
        if (p != g) ds_union(parent, g, p, words);
    }
}

// root[g] = the root of g (parent is final: the walk reads, nothing writes any more; parent[x] < x off a root)
static __global__ __launch_bounds__(256) void density_roots_kernel(const uint32_t* __restrict__ parent, uint32_t* __restrict__ root, uint32_t n) {
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n; g += gridDim.x * 256) {
        uint32_t x = g;
        for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
        root[g] = x;
    }
}

// per local row of one shard what the contract names; `from` is a global row, root [G] the flattened forest.  via /
// via_dist may be null.  The summary: a cluster is counted by the shard that holds its root.
static __global__ __launch_bounds__(256) void density_finish_sharded_kernel(const uint32_t* __restrict__ deg,
                                                                     const unsigned long long* __restrict__ bkey,
                                                                     const uint64_t* __restrict__ tomb, const uint32_t* __restrict__ root,
                                                                     uint32_t n_rows, uint32_t min_pts, IdMap map,
                                                                     uint64_t* __restrict__ cluster, uint64_t* __restrict__ via,
                                                                     float* __restrict__ via_dist, unsigned long long* __restrict__ words) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int kind = -1;   // 0 a cluster's root, 1 another core, 2 border, 3 noise
    if (r < n_rows) {
        uint64_t cl = MI_KNN_NO_ID, v = MI_KNN_NO_ID;
        float vd = __uint_as_float(0x7F800000u);
        if (!tile_dead(tomb, r)) {
            const uint32_t g = (uint32_t)id_of_local(map, r);
            const unsigned long long key = bkey[r];
            if (deg[r] >= min_pts - 1u) {
                const uint32_t x = root[g];
                cl = x; v = g; vd = 0.0f;
                kind = x == g ? 0 : 1;
            } else if (key != KEY_MAX) {
                const uint32_t from = (uint32_t)key;
                cl = root[from]; v = from; vd = u32_to_dist((uint32_t)(key >> 32));
                kind = 2;
            } else {
                kind = 3;
            }
        }
        cluster[r] = cl;
        if (via) via[r] = v;
        if (via_dist) via_dist[r] = vd;
    }
    // clusters, core rows, border rows, noise rows: lane j < 4 adds word j, one atomic instruction per wave
    const unsigned long long m0 = __ballot(kind == 0), m1 = __ballot(kind == 0 || kind == 1), m2 = __ballot(kind == 2),
                             m3 = __ballot(kind == 3);
    if (lane < 4) {
        const unsigned long long m = lane == 0 ? m0 : lane == 1 ? m1 : lane == 2 ? m2 : m3;
        if (m != 0ull) atomicAdd(words + DW_SUMMARY + lane, (unsigned long long)__popcll(m));
    }
}

}  // namespace mi

namespace {

constexpr uint32_t MERGE_CHUNK = 1u << 22;   // forest entries copied to shard 0's device at a time (16 MB)

uint32_t row_blocks(const mi_knn* t, uint64_t n) {
    return std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((uint64_t)t->n_cu * 8, (n + 255) / 256));
}

// one shard's state for the call; everything device-side lives in `scratch`, on the shard's device
struct ShardState {
    mi_knn* sh = nullptr;
    Scratch scratch;
    IdMap map{0, 0, 0, 0};
    uint32_t n_rows = 0, n_blocks = 0, cand_cap = 0;
    TableMirror tm{nullptr, nullptr, nullptr};
    uint32_t *d_deg = nullptr, *d_parent = nullptr;
    unsigned long long *d_bkey = nullptr, *d_words = nullptr;
    uint8_t* d_act = nullptr;
    uint2* d_cand = nullptr;
    DensityBlocks blocks;             // the activity bytes on the host, with their prefix counts
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ShardState() = default;
    ShardState(const ShardState&) = delete;
};

struct Params {
    float max_dist, c;
    uint32_t min_pts;   // 0: the degrees only
    uint32_t G;
};

// One piece of one pass: the row-side shard A with itself (SELF) or with the column chunk `col` of another shard.  Stage 1 is
// density_call.h's (DensityStage1: the overflow scheme and the tile counts live there); stage 2 is this unit's.
struct Piece {
    ShardState* A;
    hipStream_t s;
    Params p;
    // the column side (self: A's own arrays)
    ColChunk col;
    IdMap map_b;
    uint32_t* deg_col;
    unsigned long long* bkey_col;
    const uint8_t* d_act_col;    // the chunk's activity bytes on A's device
    CrossBlocks cross;           // ... and their prefix counts on the host

    template <int NCH, int PASS, bool SELF>
    void rect(uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) {
        mi_knn* a = A->sh;
        uint64_t* stats = A->stats;
        unsigned long long* words = A->d_words;
        DensityStage1<SELF> st1{s,
                                DensitySide{A->tm.mirror, A->tm.xx, A->tm.tomb, A->n_rows, A->d_act},
                                DensitySide{col.mirror, col.xx, col.tomb, col.n, d_act_col},
                                &A->blocks, &cross, p.c, A->cand_cap, A->d_cand, words + DW_CAND, stats};
        auto stage1 = [&](uint32_t r0, uint32_t r1, uint32_t& c0, uint32_t c1) { return st1.template stage1<NCH, PASS>(r0, r1, c0, c1); };
        auto stage2 = [&](uint32_t C) {
            const dim3 grid(group16_blocks(a, C));
            if (PASS == 1) {
                stats[0] += C;
                if (SELF)
                    hipLaunchKernelGGL((density_count_kernel<NCH>), grid, dim3(256), 0, s, a->table, A->d_cand, C, p.max_dist, A->d_deg, words);
                else
                    hipLaunchKernelGGL((density_count_between_kernel<NCH>), grid, dim3(256), 0, s, a->table, col.rows, A->map, map_b, col.off,
                                       A->d_cand, C, p.max_dist, A->d_deg, deg_col, words);
            } else {
                stats[3] += C;
                hipLaunchKernelGGL((density_link_between_kernel<NCH>), grid, dim3(256), 0, s, a->table, col.rows, A->map, map_b, col.off,
                                   A->d_cand, C, p.max_dist, p.min_pts, A->d_deg, (const uint32_t*)deg_col, A->d_parent, A->d_bkey, bkey_col,
                                   words);
            }
            HIP_CHECK(hipGetLastError());
        };
        rect_stages(br0, br1, bc0, bc1, A->cand_cap, overflowed, stage1, stage2);
    }

    // a shard with itself: the join's triangle in the join's strips
    template <int NCH, int PASS>
    void run_self() {
        tile_strips(0, A->n_blocks, 0, A->n_blocks,
                    [&](uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) { rect<NCH, PASS, true>(br0, br1, bc0, bc1, overflowed); },
                    [] { return false; });
    }
    // the chunk in `col` against all of A
    template <int NCH, int PASS>
    void run_chunk() {
        between_strips(A->n_rows, col.n, 0u, 0u,
                       [&](uint32_t br0, uint32_t br1, uint32_t bc0, uint32_t bc1, bool* overflowed) { rect<NCH, PASS, false>(br0, br1, bc0, bc1, overflowed); },
                       [] { return false; });
    }
};

// the self piece of shard x in pass PASS; x.sh->mu held, inside the shard's call frame
template <int PASS>
void self_piece(ShardState& x, const Params& p, hipStream_t s) {
    if (x.n_rows < 2) return;
    Piece pc;
    pc.A = &x; pc.s = s; pc.p = p;
    pc.col = ColChunk{x.tm.mirror, x.tm.xx, x.tm.tomb, x.sh->table, x.n_rows, 0u, 0u};
    pc.map_b = x.map;
    pc.deg_col = x.d_deg; pc.bkey_col = x.d_bkey;
    pc.d_act_col = x.d_act;
    dispatch_nch(x.sh->dim, [&](auto nch) { pc.template run_self<decltype(nch)::value, PASS>(); });
}

// Shard A (rows, where the work runs) x shard B (columns), pass PASS.  B is idle in this round.  A direct chunk works on B's
// own arrays; a staged chunk on chunk-local ones on A's device — pass 1: degrees from zero, added into B's on B's device
// behind the chunk; pass 2: a copy of B's degrees and of its activity bytes, and border keys from KEY_MAX, merged into B's by
// a minimum behind the chunk.
template <int PASS>
void cross_piece(ShardState& A, ShardState& B, const Params& p) {
    if (A.n_rows == 0 || B.n_rows == 0) return;
    mi_knn *a = A.sh, *b = B.sh;
    std::unique_lock<std::mutex> la(a->mu, std::defer_lock), lb(b->mu, std::defer_lock);
    std::lock(la, lb);
    Scratch scratch;
    TableCall call(a);
    hipStream_t s = call.s;
    b->writes.begin(s);
    b->reads.begin(s);
    ColumnWalk walk(a, b, s, scratch, &B.tm);
    Piece pc;
    pc.A = &A; pc.s = s; pc.p = p;
    pc.map_b = B.map;
    uint32_t* st_deg = nullptr;
    unsigned long long* st_bkey = nullptr;
    uint8_t* st_act = nullptr;
    void* d_in = nullptr;   // on B's device: where a staged chunk's array lands before it is merged
    hipStream_t sb = nullptr;
    if (walk.staged) {
        st_deg = (uint32_t*)scratch.get((size_t)walk.chunk_rows * sizeof(uint32_t));
        if (PASS == 2) {
            st_bkey = (unsigned long long*)scratch.get((size_t)walk.chunk_rows * sizeof(unsigned long long));
            st_act = (uint8_t*)scratch.get(walk.chunk_rows / TILE);
        }
        DeviceGuard gb(b->device);
        d_in = scratch.get((size_t)walk.chunk_rows * (PASS == 1 ? sizeof(uint32_t) : sizeof(unsigned long long)));
        sb = knn_own_stream(b);
    }
    for (uint32_t ci = 0; ci < walk.n_chunks; ++ci) {
        uint64_t c0, c1;
        between_chunk(b->rows, walk.chunk_rows, ci, &c0, &c1);
        const uint32_t cn = (uint32_t)(c1 - c0), nb = between_tiles_of(cn);
        const uint8_t* h_act_col = nullptr;
        if (PASS == 2) {
            // nothing to visit in the whole chunk: it is not staged either
            h_act_col = B.blocks.act.data() + c0 / TILE;
            pc.cross.index(h_act_col, nb);
            uint64_t visited = 0, skipped = 0;
            pc.cross.count(A.blocks.act.data(), 0, A.n_blocks, 0, nb, &visited, &skipped);
            if (visited == 0) { A.stats[5] += skipped; continue; }
        }
        walk.chunk(ci, A.n_rows, 0u, 0u, &pc.col);
        if (!walk.staged) {
            pc.deg_col = B.d_deg + c0;
            pc.bkey_col = B.d_bkey ? B.d_bkey + c0 : nullptr;
            pc.d_act_col = B.d_act ? B.d_act + c0 / TILE : nullptr;
        } else if (PASS == 1) {
            HIP_CHECK(hipMemsetAsync(st_deg, 0, (size_t)cn * sizeof(uint32_t), s));
            pc.deg_col = st_deg;
        } else {
            copy_between(st_deg, a->device, B.d_deg + c0, b->device, (size_t)cn * sizeof(uint32_t), s);
            HIP_CHECK(hipMemsetAsync(st_bkey, 0xFF, (size_t)cn * sizeof(unsigned long long), s));
            HIP_CHECK(hipMemcpyAsync(st_act, h_act_col, nb, hipMemcpyHostToDevice, s));
            pc.deg_col = st_deg; pc.bkey_col = st_bkey; pc.d_act_col = st_act;
        }
        dispatch_nch(a->dim, [&](auto nch) { pc.template run_chunk<decltype(nch)::value, PASS>(); });
        HIP_CHECK(hipStreamSynchronize(s));   // (staged: the scratch and h_tomb are free for the next chunk)
        if (walk.staged) {
            DeviceGuard gb(b->device);
            if (PASS == 1) {
                copy_between(d_in, b->device, st_deg, a->device, (size_t)cn * sizeof(uint32_t), sb);
                hipLaunchKernelGGL(density_add_kernel, dim3(row_blocks(b, cn)), dim3(256), 0, sb, B.d_deg + c0, (const uint32_t*)d_in, cn);
            } else {
                copy_between(d_in, b->device, st_bkey, a->device, (size_t)cn * sizeof(unsigned long long), sb);
                hipLaunchKernelGGL(density_min_kernel, dim3(row_blocks(b, cn)), dim3(256), 0, sb, B.d_bkey + c0,
                                   (const unsigned long long*)d_in, cn);
            }
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(sb));
        }
    }
}

template <int PASS>
void cross_rounds(ShardedCall& call, std::vector<std::unique_ptr<ShardState>>& st, const Params& p) {
    for (const std::vector<ShardPair>& round : between_schedule(call.n))
        call.for_each_shard_pair(round, [&](uint32_t ra, uint32_t cb) { cross_piece<PASS>(*st[ra], *st[cb], p); });
}

struct ShardedDensityOut {
    std::vector<uint64_t> cluster, via;
    std::vector<float> via_dist;
    std::vector<uint32_t> counts;
    uint64_t summary[4] = {0, 0, 0, 0};
};

// min_pts == 0: the degrees only (mi_knn_sharded_density).  Everything lands in `out`, by global row; the caller's arrays are
// written by the caller once the frame has left.
void sharded_density_run(ShardedCall& call, float max_dist, uint32_t min_pts, bool want_via, bool want_via_dist, bool want_counts,
                         ShardedDensityOut* out) {
    mi_knn_sharded* t = call.t;
    for (uint64_t& v : t->dbscan_stats) v = 0;
    check_mirror_dim(t->dim, "the density pass's");
    if (!sharded_density_rows_ok(t->rows)) fail(MI_ERR_UNSUPPORTED, "at most 2^32 - 1 rows (got %llu)", (unsigned long long)t->rows);
    call.ready();
    const uint64_t G = t->rows;
    if (G == 0) return;
    const uint32_t S = call.n;
    const Params p{max_dist, 1.0f - (max_dist + eps2(t->dim)), min_pts, (uint32_t)G};
    std::vector<std::unique_ptr<ShardState>> st(S);
    for (uint32_t si = 0; si < S; ++si) st[si].reset(new ShardState);

    // the shards' state and their self pieces of pass 1, side by side
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        std::lock_guard<std::mutex> l(sh->mu);
        ShardState& x = *st[si];
        x.sh = sh;
        x.n_rows = (uint32_t)sh->rows;
        x.n_blocks = between_tiles_of(sh->rows);
        x.map = knn_id_map(sh);
        if (x.n_rows == 0) return;
        TableCall call(sh);
        hipStream_t s = call.s;
        x.cand_cap = std::max<uint32_t>(TILE_CAP_MIN, sh->join_cap);
        x.d_deg = (uint32_t*)x.scratch.get((size_t)x.n_rows * sizeof(uint32_t));
        x.d_words = (unsigned long long*)x.scratch.get(DW_WORDS * sizeof(unsigned long long));
        x.d_cand = (uint2*)x.scratch.get((size_t)x.cand_cap * sizeof(uint2));
        HIP_CHECK(hipMemsetAsync(x.d_deg, 0, (size_t)x.n_rows * sizeof(uint32_t), s));
        HIP_CHECK(hipMemsetAsync(x.d_words, 0, DW_WORDS * sizeof(unsigned long long), s));
        if (min_pts != 0) {
            x.d_bkey = (unsigned long long*)x.scratch.get((size_t)x.n_rows * sizeof(unsigned long long));
            x.d_act = (uint8_t*)x.scratch.get(x.n_blocks);
            x.d_parent = (uint32_t*)x.scratch.get((size_t)G * sizeof(uint32_t));
            hipLaunchKernelGGL(density_forest_init_kernel, dim3(row_blocks(sh, G)), dim3(256), 0, s, x.d_parent, p.G);
            HIP_CHECK(hipGetLastError());
        }
        x.tm = table_mirror(sh, s, x.scratch);
        self_piece<1>(x, p, s);
    });
    cross_rounds<1>(call, st, p);

    if (min_pts == 0) {
        out->counts.assign(G, 0u);
        call.for_each_shard([&](uint32_t si, mi_knn* sh) {
            ShardState& x = *st[si];
            if (x.n_rows == 0) return;
            std::lock_guard<std::mutex> l(sh->mu);
            TableCall call(sh);
            std::vector<uint32_t> deg(x.n_rows);
            unsigned long long words[DW_WORDS];
            HIP_CHECK(hipMemcpyAsync(deg.data(), x.d_deg, (size_t)x.n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, call.s));
            HIP_CHECK(hipMemcpyAsync(words, x.d_words, sizeof words, hipMemcpyDeviceToHost, call.s));
            HIP_CHECK(hipStreamSynchronize(call.s));
            x.stats[1] = words[DW_WITHIN];
            scatter_to_global(x.map, deg.data(), x.n_rows, out->counts.data());
        });
        for (uint32_t si = 0; si < S; ++si)
            for (int i = 0; i < 8; ++i) t->dbscan_stats[i] += st[si]->stats[i];
        return;
    }

    // between the passes: the activity bytes and the border keys' init, then the self pieces of pass 2
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        ShardState& x = *st[si];
        if (x.n_rows == 0) return;
        std::lock_guard<std::mutex> l(sh->mu);
        TableCall call(sh);
        hipStream_t s = call.s;
        // (parent: the kernel writes r into entry r of the shard's first local-row-count entries, which is what the forest
        // holds there already)
        hipLaunchKernelGGL(density_blocks_kernel, dim3(x.n_blocks), dim3(TILE), 0, s, x.d_deg, x.tm.tomb, x.n_rows, min_pts, x.d_parent,
                           x.d_bkey, x.d_act);
        HIP_CHECK(hipGetLastError());
        x.blocks.act.resize(x.n_blocks);
        HIP_CHECK(hipMemcpyAsync(x.blocks.act.data(), x.d_act, x.n_blocks, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        x.blocks.index();
        self_piece<2>(x, p, s);
    });
    cross_rounds<2>(call, st, p);

    // forest s into forest 0 on shard 0's device (shard 0 holds row 0: it is not empty), the roots, and the roots back
    uint32_t* d_root = nullptr;
    {
        ShardState& z = *st[0];
        std::lock_guard<std::mutex> l(z.sh->mu);
        TableCall call(z.sh);
        hipStream_t s = call.s;
        uint32_t* d_in = (uint32_t*)z.scratch.get((size_t)std::min<uint64_t>(G, MERGE_CHUNK) * sizeof(uint32_t));
        d_root = (uint32_t*)z.scratch.get((size_t)G * sizeof(uint32_t));
        for (uint32_t si = 1; si < S; ++si) {
            if (st[si]->n_rows == 0) continue;
            for (uint64_t g0 = 0; g0 < G; g0 += MERGE_CHUNK) {
                const uint32_t n = (uint32_t)std::min<uint64_t>(MERGE_CHUNK, G - g0);
                copy_between(d_in, z.sh->device, st[si]->d_parent + g0, st[si]->sh->device, (size_t)n * sizeof(uint32_t), s);
                hipLaunchKernelGGL(density_forest_merge_kernel, dim3(row_blocks(z.sh, n)), dim3(256), 0, s, z.d_parent, (const uint32_t*)d_in,
                                   (uint32_t)g0, n, z.d_words);
                HIP_CHECK(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(density_roots_kernel, dim3(row_blocks(z.sh, G)), dim3(256), 0, s, (const uint32_t*)z.d_parent, d_root, p.G);
        HIP_CHECK(hipGetLastError());
        // (a shard's own forest has been merged: its memory takes the roots)
        for (uint32_t si = 1; si < S; ++si)
            if (st[si]->n_rows != 0) copy_between(st[si]->d_parent, st[si]->sh->device, d_root, z.sh->device, (size_t)G * sizeof(uint32_t), s);
        HIP_CHECK(hipStreamSynchronize(s));
    }

    // every shard resolves its local rows; the host scatters them to global rows
    ShardedDensityOut res;
    res.cluster.assign(G, MI_KNN_NO_ID);
    if (want_via) res.via.assign(G, MI_KNN_NO_ID);
    if (want_via_dist) res.via_dist.assign(G, 0.0f);
    if (want_counts) res.counts.assign(G, 0u);
    std::vector<unsigned long long> words((size_t)S * DW_WORDS, 0ull);
    call.for_each_shard([&](uint32_t si, mi_knn* sh) {
        ShardState& x = *st[si];
        if (x.n_rows == 0) return;
        std::lock_guard<std::mutex> l(sh->mu);
        TableCall call(sh);
        hipStream_t s = call.s;
        const size_t n = x.n_rows;
        uint64_t* d_cluster = (uint64_t*)x.scratch.get(n * sizeof(uint64_t));
        uint64_t* d_via = want_via ? (uint64_t*)x.scratch.get(n * sizeof(uint64_t)) : nullptr;
        float* d_via_dist = want_via_dist ? (float*)x.scratch.get(n * sizeof(float)) : nullptr;
        hipLaunchKernelGGL(density_finish_sharded_kernel, dim3((x.n_rows + 255) / 256), dim3(256), 0, s, (const uint32_t*)x.d_deg,
                           (const unsigned long long*)x.d_bkey, x.tm.tomb, (const uint32_t*)(si == 0 ? d_root : x.d_parent), x.n_rows, min_pts,
                           x.map, d_cluster, d_via, d_via_dist, x.d_words);
        HIP_CHECK(hipGetLastError());
        std::vector<uint64_t> cluster(n), via(want_via ? n : 0);
        std::vector<float> via_dist(want_via_dist ? n : 0);
        std::vector<uint32_t> deg(want_counts ? n : 0);
        HIP_CHECK(hipMemcpyAsync(words.data() + (size_t)si * DW_WORDS, x.d_words, DW_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(cluster.data(), d_cluster, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (want_via) HIP_CHECK(hipMemcpyAsync(via.data(), d_via, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (want_via_dist) HIP_CHECK(hipMemcpyAsync(via_dist.data(), d_via_dist, n * sizeof(float), hipMemcpyDeviceToHost, s));
        if (want_counts) HIP_CHECK(hipMemcpyAsync(deg.data(), x.d_deg, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        scatter_to_global(x.map, cluster.data(), n, res.cluster.data());
        if (want_via) scatter_to_global(x.map, via.data(), n, res.via.data());
        if (want_via_dist) scatter_to_global(x.map, via_dist.data(), n, res.via_dist.data());
        if (want_counts) scatter_to_global(x.map, deg.data(), n, res.counts.data());
    });
    unsigned long long errors = 0;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t si = 0; si < S; ++si) {
        const unsigned long long* w = words.data() + (size_t)si * DW_WORDS;
        errors += w[DW_ERROR];
        for (int i = 0; i < 4; ++i) res.summary[i] += w[DW_SUMMARY + i];
        for (int i = 0; i < 8; ++i) stats[i] += st[si]->stats[i];
        stats[1] += w[DW_WITHIN];
        stats[6] += w[DW_MERGED];
    }
    if (errors != 0)
        fail(MI_ERR_HIP, "internal error: a step cap of the disjoint-set forest expired (%llu times); nothing was written", errors);
    for (int i = 0; i < 8; ++i) t->dbscan_stats[i] = stats[i];
    *out = std::move(res);
}

}  // namespace

extern "C" {

int mi_knn_sharded_density(mi_knn_sharded* t, float max_dist, uint32_t* counts) {
    return guarded([&] {
        const char* why = "";
        const int bad = density_check_args(t, max_dist, counts, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        ShardedDensityOut out;
        {
            ShardedCall call(t);
            sharded_density_run(call, max_dist, 0, false, false, true, &out);
        }
        copy_out(out.counts, counts);
    });
}

int mi_knn_sharded_dbscan(mi_knn_sharded* t, float max_dist, uint32_t min_pts, uint64_t* cluster, uint64_t* via, float* via_dist,
                          uint32_t* counts, uint64_t summary[4]) {
    return guarded([&] {
        const char* why = "";
        const int bad = dbscan_check_args(t, max_dist, min_pts, cluster, summary, &why);
        if (bad != MI_OK) fail(bad, "%s", why);
        ShardedDensityOut out;
        {
            ShardedCall call(t);
            sharded_density_run(call, max_dist, min_pts, via != nullptr, via_dist != nullptr, counts != nullptr, &out);
        }
        copy_out(out.cluster, cluster);
        copy_out(out.via, via);
        copy_out(out.via_dist, via_dist);
        copy_out(out.counts, counts);
        for (int i = 0; i < 4; ++i) summary[i] = out.summary[i];
    });
}

int mi_knn_sharded_dbscan_stats(mi_knn_sharded* t, uint64_t out[8]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 8; ++i) out[i] = t->dbscan_stats[i];
    });
}

}  // extern "C"
