// where_pred.h — the predicate of the *_where calls on the device: the structure the kernels take, how the public one becomes
// it, and the test of one row.  where_kernels.h compacts the qualifying rows into a list with it; search_many_where_kernels.h
// turns it into a bitmap.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mi355clip.h"

namespace mi {

// the predicate as the kernels take it (mi_knn_where, with the flag decoded); tags / stamps / groups / tomb are nullable:
// a table without attribute columns holds the defaults (0, 0), one without deletions has no bitmap, and the group word is
// read only under the flag (the host answers "nothing" itself when the flag is set and there is no column)
struct WherePred {
    unsigned long long all_of, any_of, none_of;
    long long lo, hi;
    uint32_t group, use_group;
};
// (host) the public predicate, checked by the caller (where_host.h), in that form
inline WherePred pred_of(const mi_knn_where& w) {
    WherePred p;
    p.all_of = w.all_of; p.any_of = w.any_of; p.none_of = w.none_of;
    p.lo = w.stamp_lo; p.hi = w.stamp_hi;
    p.group = w.group;
    p.use_group = (w.flags & MI_KNN_WHERE_GROUP) ? 1u : 0u;
    return p;
}

__device__ __forceinline__ bool where_match(const WherePred& p, const unsigned long long* __restrict__ tags,
                                            const long long* __restrict__ stamps, const uint32_t* __restrict__ groups,
                                            const unsigned long long* __restrict__ tomb, uint64_t row, uint64_t rows) {
    if (row >= rows) return false;
    const unsigned long long tg = tags ? tags[row] : 0ull;
    const long long st = stamps ? stamps[row] : 0ll;
    bool ok = (tg & p.all_of) == p.all_of && (p.any_of == 0ull || (tg & p.any_of) != 0ull) && (tg & p.none_of) == 0ull;
    ok = ok && st >= p.lo && st <= p.hi;
    if (tomb) ok = ok && ((tomb[row >> 6] >> (row & 63)) & 1ull) == 0ull;   // one word per tile: the same address in all 64 lanes
    if (p.use_group) ok = ok && groups[row] == p.group;
    return ok;
}

}  // namespace mi
