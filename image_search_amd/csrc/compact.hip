// compact.hip — mi_knn_compact: the deleted rows leave the table physically, the survivors close up in order and take new
// ids.  The moves and why they are safe: compact_kernels.h.  The map, the chunk plan and the host columns: compact_host.h.
//
// One call: the sorted list of deleted rows goes up (4 bytes per deleted row), compact_src_kernel turns it into the source row
// of every destination row from the first deleted row on (4 bytes per such row), then per chunk one compact_move_kernel
// launch (straight) or two (staged), then per column that exists one compact_gather_kernel into a call-private buffer, a copy
// back and a fill of the freed tail, then the tombstone bitmap is zeroed — all on the handle's stream, waited for once.  Extra
// device memory: the two lists, the staging buffer (one chunk) and one column temporary (8 bytes per moved row); never a
// second table.  Everything is checked and allocated before the first row moves; a HIP error after that leaves the rows
// partly moved and the call says so.
#include <algorithm>

#include <mutex>
#include <vector>

#include "common.h"
#include "compact_host.h"
#include "compact_kernels.h"
#include "handles.h"

using namespace mi;

namespace {

uint32_t compact_grid(const mi_knn* t, uint64_t work) {
    const uint64_t blocks = (work + COMPACT_THREADS - 1) / COMPACT_THREADS;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(t->n_cu, 1) * 16));
}

void launch_move(const mi_knn* t, const float* src, float* dst, const uint32_t* rows, uint64_t n_rows, hipStream_t s) {
    const uint32_t pieces = t->dim / 4;
    if (n_rows * pieces > COMPACT_MAX_PIECES) fail(MI_ERR_INVALID, "a chunk of %llu rows is more than one launch moves", (unsigned long long)n_rows);
    hipLaunchKernelGGL(compact_move_kernel, dim3(compact_grid(t, n_rows * pieces)), dim3(COMPACT_THREADS), 0, s,
                       reinterpret_cast<const compact_v4f*>(src), reinterpret_cast<compact_v4f*>(dst), rows, (uint32_t)n_rows, pieces);
    HIP_CHECK(hipGetLastError());
}

// the device half of a column (one that exists): col[first .. first + n) = col[rows[..]] through tmp, then the freed tail
// [first + n, old_rows) = the default
template <class T>
void compact_device_column(const mi_knn* t, RowColumn<T>& col, const uint32_t* d_src, uint64_t first, uint64_t n, uint64_t old_rows, void* tmp,
                           hipStream_t s) {
    if (!col.p) return;
    if (n) {
        hipLaunchKernelGGL(compact_gather_kernel<T>, dim3(compact_grid(t, n)), dim3(COMPACT_THREADS), 0, s, (const T*)col.p, d_src, (uint32_t)n, (T*)tmp);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(col.p + first, tmp, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, s));
    }
    const uint64_t end = std::min<uint64_t>(old_rows, col.cap);
    if (end > first + n) HIP_CHECK(hipMemsetAsync(col.p + first + n, col.fill, (size_t)(end - first - n) * sizeof(T), s));
}

}  // namespace

extern "C" {

int mi_knn_compact(mi_knn* t, uint64_t* new_ids, uint64_t cap, uint64_t* removed) {
    return guarded([&] {
        if (!t) fail(MI_ERR_INVALID, "null table handle");
        std::lock_guard<std::mutex> l(t->mu);
        if (t->cyc_n > 1) fail(MI_ERR_UNSUPPORTED, "a shard of a sharded table cannot be compacted: its ids are not its own to renumber (mi_knn_sharded_compact_into)");
        const uint64_t rows = t->rows;
        if (new_ids && cap < rows) fail(MI_ERR_INVALID, "new_ids holds %llu entries, the table %llu rows", (unsigned long long)cap, (unsigned long long)rows);
        const std::vector<uint32_t>& dead = t->dead;
        if (dead.empty()) {   // nothing to reclaim: nothing is launched, nothing changes
            if (new_ids) compact_map(dead, rows, t->base, new_ids);
            if (removed) *removed = 0;
            for (uint64_t& w : t->compact_stats) w = 0;
            return;
        }
        const CompactPlan plan = compact_plan(dead, rows, compact_chunk_rows(t->compact_chunk_rows, t->dim));
        const uint64_t n_dead = dead.size(), n_move = plan.live - plan.first;
        const size_t row_elems = t->dim;
        // the host columns as they will be, built aside: nothing of the handle changes before the device work has run
        std::vector<uint32_t> h_groups = t->d_groups.host;
        std::vector<uint64_t> h_tags = t->d_tags.host;
        std::vector<int64_t> h_stamps = t->d_stamps.host;
        compact_column(h_groups, dead);
        compact_column(h_tags, dead);
        compact_column(h_stamps, dead);
        uint64_t n_grouped = 0;
        for (uint32_t g : h_groups) n_grouped += g != MI_KNN_NO_GROUP;

        Scratch scratch;   // declared before the device guard: freed after the stream has gone idle
        DeviceGuard g(t->device);
        hipStream_t s = knn_own_stream(t);
        uint32_t* d_sorted = nullptr;
        uint32_t* d_src = nullptr;
        float* d_stage = nullptr;
        void* d_col = nullptr;
        if (n_move) {
            d_sorted = (uint32_t*)scratch.get((size_t)n_dead * sizeof(uint32_t));
            d_src = (uint32_t*)scratch.get((size_t)n_move * sizeof(uint32_t));
            if (plan.stage_rows) d_stage = (float*)scratch.get((size_t)plan.stage_rows * row_elems * sizeof(float));
            if (t->d_groups || t->d_tags || t->d_stamps) d_col = scratch.get((size_t)n_move * sizeof(uint64_t));
        }
        // the rows move: everything enqueued against them, on whichever stream, must have finished (as for grow())
        t->writes.sync();
        t->reads.sync();
        if (n_move) {
            HIP_CHECK(hipMemcpyAsync(d_sorted, dead.data(), (size_t)n_dead * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(compact_src_kernel, dim3(compact_grid(t, n_move)), dim3(COMPACT_THREADS), 0, s, (const uint32_t*)d_sorted,
                               (uint32_t)n_dead, (uint32_t)plan.first, (uint32_t)n_move, d_src);
            HIP_CHECK(hipGetLastError());
            for (const CompactChunk& c : plan.chunks) {
                const uint32_t* list = d_src + (c.j0 - plan.first);
                float* place = t->table + c.j0 * row_elems;
                if (!c.staged) launch_move(t, t->table, place, list, c.j1 - c.j0, s);
                else {
                    launch_move(t, t->table, d_stage, list, c.j1 - c.j0, s);
                    launch_move(t, d_stage, place, nullptr, c.j1 - c.j0, s);
                }
            }
        }
        // the columns by the same list, out of place; then their freed tails hold the defaults (knn_truncate's guarantee)
        compact_device_column(t, t->d_groups, d_src, plan.first, n_move, rows, d_col, s);
        compact_device_column(t, t->d_tags, d_src, plan.first, n_move, rows, d_col, s);
        compact_device_column(t, t->d_stamps, d_src, plan.first, n_move, rows, d_col, s);
        if (t->d_tomb) HIP_CHECK(hipMemsetAsync(t->d_tomb, 0, t->d_tomb.cap * sizeof(uint64_t), s));
        const hipError_t done = hipStreamSynchronize(s);
        if (done != hipSuccess) fail(MI_ERR_HIP, "the compaction failed on the device (%s): the table's rows are partly moved", hipGetErrorString(done));

        // the handle: a table of `live` rows without deletions
        if (new_ids) compact_map(dead, rows, t->base, new_ids);
        if (removed) *removed = n_dead;
        t->compact_stats[0] = n_dead; t->compact_stats[1] = n_move;
        t->compact_stats[2] = plan.n_straight; t->compact_stats[3] = plan.n_staged;
        t->rows = plan.live;
        t->mirror_rows = std::min(t->mirror_rows, plan.first);   // the next search mirrors the moved rows again
        t->d_groups.host.swap(h_groups);
        t->d_tags.host.swap(h_tags);
        t->d_stamps.host.swap(h_stamps);
        t->n_grouped = n_grouped;
        ++t->groups_epoch;
        t->gslots_valid = false;
        t->n_flist = 0;
        t->last_prefiltered = false;
        t->dead.clear();
        t->d_dead.release();
    });
}

int mi_knn_compact_stats(mi_knn* t, uint64_t out[4]) {
    return guarded([&] {
        if (!t || !out) fail(MI_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> l(t->mu);
        for (int i = 0; i < 4; ++i) out[i] = t->compact_stats[i];
    });
}

}  // extern "C"
