// scan_call.h — what the calls that read the table on the handle's own stream share on the host: the frame of such a call
// (TableCall), and for the single-query scans (page, compound, grouped, ordered, the stamp histogram) the candidate set, the
// selection of the k best keys, the one record that goes back, the grid rule and the dim rule.  The per-call argument rules,
// records, scans and finish kernels stay with the calls: they are the contracts.
//
// The first part holds rules without HIP in them; a host compiler sees that part alone (tests/cpp/test_page_host.cpp and
// test_compound_host.cpp run it under the sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>

#include "error.h"

namespace mi {

constexpr uint32_t SCAN_K_MAX = 4096;   // what the selection below delivers at most

// the dims the scans (and the bf16 mirror of two_stage.h) are built for
inline bool scan_dim_ok(uint32_t dim) { return dim == 128 || dim == 256 || dim == 512 || dim == 768 || dim == 1024; }
// `what`: "the paged search", "the join's bf16 mirror", ... for the message
inline void check_scan_dim(uint32_t dim, const char* what) {
    if (!scan_dim_ok(dim)) fail(MI_ERR_UNSUPPORTED, "dim %u: %s is built for dim in {128, 256, 512, 768, 1024}", dim, what);
}

// workgroups of a scan over n rows or list entries (a workgroup = 4 waves, a wave's tile = 64): option 0 = per_cu per CU,
// v >= 1 = exactly min(v, needed)
inline uint32_t scan_grid(uint64_t n, int n_cu, int option, uint32_t per_cu) {
    const uint64_t n_tiles = (n + 63) / 64, needed = std::max<uint64_t>(1, (n_tiles + 3) / 4);
    const uint64_t want = option >= 1 ? (uint64_t)option : (uint64_t)std::max(n_cu, 1) * per_cu;
    return (uint32_t)std::min(want, needed);
}

}  // namespace mi

#ifdef __HIPCC__
#include <initializer_list>
#include <vector>

#include "common.h"
#include "handles.h"

namespace mi {

// whatever happens, the handle's stream is idle and its order words say so when the call leaves
struct Settle {
    mi_knn* t; hipStream_t s;
    ~Settle() { (void)hipStreamSynchronize(s); t->reads.pending = false; }
};

// The frame of a call that reads the table on the handle's own stream, t->mu held: the device selected, the stream ordered
// behind every write and search enqueued before this call (on whichever stream), and settled on every way out.  Device memory
// of the call alone (Scratch) is declared BEFORE the frame, so that it is freed after the stream has gone idle (hipFree finds
// the memory's device by itself, whichever is selected by then).
//
// The handle's workspace is reserved AFTER the frame opens (DevArray::reserve on t->reads; knn_select_keys32 and knn_filter_where do the same).  That is
// the same as reserving in front of it: reserve touches the order words only when it must grow a buffer, and then waits
// on the host for the searches in flight (reads.sync) before it frees — the wait the stream has just been given (reads.begin)
// is then a wait for an event that has fired, and reads.pending is false either way.  Writes never use the workspace.
struct TableCall {
    mi_knn* t;
    DeviceGuard g;
    hipStream_t s;
    explicit TableCall(mi_knn* table) : t(table), g(table->device), s(knn_own_stream(table)) {
        t->writes.begin(s);
        t->reads.begin(s);
    }
    TableCall(const TableCall&) = delete;
    ~TableCall() { (void)hipStreamSynchronize(s); t->reads.pending = false; }
};

// A write to columns the host holds too (the group column, the attribute columns), inside the frame: the span of rows the call
// names (`rows`, not empty) goes up in one copy per column, behind the searches enqueued before this call and ahead of every
// later one (writes.end), and is waited for.  A column whose device pointer is null is left out.
struct ColumnSpan {
    void* dev; const void* host; size_t elem;
};
inline void upload_span(TableCall& call, const std::vector<uint32_t>& rows, std::initializer_list<ColumnSpan> cols) {
    const auto ends = std::minmax_element(rows.begin(), rows.end());
    const uint32_t lo = *ends.first, hi = *ends.second;
    for (const ColumnSpan& c : cols)
        if (c.dev)
            HIP_CHECK(hipMemcpyAsync((char*)c.dev + (size_t)lo * c.elem, (const char*)c.host + (size_t)lo * c.elem,
                                     ((size_t)(hi - lo) + 1) * c.elem, hipMemcpyHostToDevice, call.s));
    call.t->writes.end(call.s);
    HIP_CHECK(hipStreamSynchronize(call.s));
}

// ---- the candidates of a scan -------------------------------------------------------------------------------------------
// SCAN_TABLE: every row under the deletion bitmap.  SCAN_HOST_IDS: the list knn_filter_rows left in t->h_flist (every id
// checked, deleted rows left out) — it goes up on s here.  SCAN_DEVICE_LIST: the list knn_filter_where left in t->d_flist.
// A list holds live rows only, so no bitmap goes with it.  A call whose candidates are known on the host (the first two
// kinds) leaves with its padding before any device work when scan_count is 0.
enum ScanFrom { SCAN_TABLE, SCAN_HOST_IDS, SCAN_DEVICE_LIST };
struct ScanSet {
    uint64_t n;
    const uint32_t* list;
    const uint64_t* tomb;
};
inline uint64_t scan_count(const mi_knn* t, ScanFrom from) { return from == SCAN_TABLE ? t->rows : (uint64_t)t->n_flist; }
inline ScanSet scan_set(mi_knn* t, hipStream_t s, ScanFrom from) {
    if (from == SCAN_TABLE) return ScanSet{t->rows, nullptr, t->dead.empty() ? nullptr : t->d_tomb};
    if (from == SCAN_HOST_IDS) knn_filter_upload(t, s);
    return ScanSet{(uint64_t)t->n_flist, t->d_flist, nullptr};
}

// ---- the selection of the k <= 4096 best keys ---------------------------------------------------------------------------
// the radix select's half alone: room for one 32-bit key per row or list entry (what knn_select_keys32 reads) and for the k
// best in t->d_keys
inline uint32_t* scan_keys32(mi_knn* t, uint64_t n) {
    t->d_keys.reserve(t->reads, (size_t)SCAN_K_MAX);
    t->d_keys32.reserve(t->reads, (size_t)std::max<uint64_t>(n, t->cap));
    return t->d_keys32;
}
// k <= 64: the scan's waves keep lists of k keys (cand, `lists` of them), reduced by the search's merge tree; above: the scan
// leaves one key per entry (all_keys) for the search's radix select.  Either way the k best land in t->d_keys, ascending.
struct ScanSelect {
    uint64_t n;
    uint32_t k, lists;
    uint64_t* cand;       // what the scan is handed: one of the two is null
    uint32_t* all_keys;
};
inline ScanSelect scan_select_reserve(mi_knn* t, uint64_t n, uint32_t k, uint32_t lists) {
    if (k > 64) return ScanSelect{n, k, lists, nullptr, scan_keys32(t, n)};
    t->d_keys.reserve(t->reads, (size_t)SCAN_K_MAX);
    t->d_cand.reserve(t->reads, (size_t)lists * k);
    return ScanSelect{n, k, lists, t->d_cand, nullptr};
}
inline void scan_select(mi_knn* t, const ScanSelect& sel, const uint32_t* list, hipStream_t s) {
    if (sel.k <= 64) knn_reduce_lists64(t, sel.lists, sel.k, t->d_keys, s);
    else knn_select_keys32(t, sel.n, sel.k, t->d_keys, list, s);
}

// ---- the one record a call leaves on the device (in t->d_idx) and copies back in one piece -------------------------------
inline unsigned char* scan_record(mi_knn* t, size_t bytes) {
    t->d_idx.reserve(t->reads, (bytes + 7) / 8);
    return reinterpret_cast<unsigned char*>(t->d_idx.p);
}
// its first `bytes` on the host, once everything enqueued on s has run
inline std::vector<unsigned char> scan_record_fetch(const unsigned char* d_rec, size_t bytes, hipStream_t s) {
    std::vector<unsigned char> h_rec(bytes);
    HIP_CHECK(hipMemcpyAsync(h_rec.data(), d_rec, bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return h_rec;
}

}  // namespace mi
#endif  // __HIPCC__
