// representatives_host.h — the host-only rules of mi_knn_representatives (representatives.hip): the argument check, the
// 64-bit word a group's candidates are folded into and how it is read, the min_gap window on keys, how the per-group arrays
// turn into ids and distances, the translation of `start`, and the padding of an empty table.  The word and the window are
// marked for both sides when a HIP compiler reads this file (representatives_kernels.h uses them); nothing else in here knows
// of HIP: tests/cpp/test_representatives_host.cpp runs it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/mi355clip.h"
#include "ids.h"
#include "summary_host.h"

namespace mi {

constexpr uint32_t REP_MAX_C = SUMMARY_MAX_C, REP_MAX_M = 4096, REP_MAX_CM = 1u << 22;
constexpr uint32_t REP_NO_ROW = 0xFFFFFFFFu;   // "no local row": the padding of picks, a start id that is no row of the table
constexpr uint32_t REP_CHECK_EVERY = 8;        // rounds enqueued between two looks at "did the last round pick anything"

// MI_OK, or the code with *why set: the handle, C, m, their product, min_gap.  Judged before the handle is followed.
inline int rep_check_args(const void* t, uint32_t C, uint32_t m, float min_gap, const char** why) {
    *why = "";
    if (!t) { *why = "null table handle"; return MI_ERR_INVALID; }
    if (C == 0) { *why = "C must be >= 1"; return MI_ERR_INVALID; }
    if (m == 0) { *why = "m must be >= 1"; return MI_ERR_INVALID; }
    if (min_gap != min_gap) { *why = "min_gap is NaN"; return MI_ERR_INVALID; }
    if (C > REP_MAX_C) { *why = "at most 65536 groups"; return MI_ERR_UNSUPPORTED; }
    if (m > REP_MAX_M) { *why = "at most 4096 picks per group"; return MI_ERR_UNSUPPORTED; }
    if ((uint64_t)C * m > REP_MAX_CM) { *why = "C * m is at most 2^22"; return MI_ERR_UNSUPPORTED; }
    return MI_OK;
}

// A group's candidates of one round fold into ONE word by a 64-bit max: (K << 32) | (0xFFFFFFFF - local row) — the largest key
// wins, among equal keys the LOWEST row (= the lowest id: local rows ascend with their ids, ids.h).  Only number keys are
// folded, and no number has key 0 (that would be the bits of a negative NaN, and every NaN's key is 0xFFFFFFFF), so a real
// word is >= 2^32 and 0 says "no candidate".  Two shards' words for one group merge by the same max once the rows are global.
constexpr uint64_t REP_SLOT_EMPTY = 0ull;
MI_IDS_HD inline uint64_t rep_word(uint32_t key, uint32_t row) { return ((uint64_t)key << 32) | (uint32_t)(0xFFFFFFFFu - row); }
MI_IDS_HD inline uint32_t rep_word_key(uint64_t w) { return (uint32_t)(w >> 32); }
MI_IDS_HD inline uint32_t rep_word_row(uint64_t w) { return 0xFFFFFFFFu - (uint32_t)w; }

// the window of min_gap, on keys: a candidate is taken iff its key is ABOVE key(min_gap); -inf = no bound at all
struct RepWindow { uint32_t key, bounded; };
inline RepWindow rep_window(float min_gap) {
    RepWindow w;
    w.key = summary_key_of(min_gap);
    w.bounded = (std::isinf(min_gap) && min_gap < 0.0f) ? 0u : 1u;
    return w;
}
MI_IDS_HD inline bool rep_takes(uint64_t word, uint32_t window_key, uint32_t bounded) {
    return word != REP_SLOT_EMPTY && (!bounded || rep_word_key(word) > window_key);
}

// start [C] ids -> local rows for the device (REP_NO_ROW where the id is no row of the table: the device refuses it if the
// group has a member)
inline void rep_start_rows(const IdMap& map, uint64_t rows, const uint64_t* start, uint32_t C, uint32_t* out) {
    for (uint32_t c = 0; c < C; ++c) {
        uint64_t local = 0;
        out[c] = (local_of_id(map, rows, start[c], &local) && local < REP_NO_ROW) ? (uint32_t)local : REP_NO_ROW;
    }
}

// the device's per-group arrays -> the caller's (each may be null).  rows [C][m] local rows (REP_NO_ROW = none), gaps [C][m],
// n [C], reach_word [C]: the 64-bit max of rep_word(K, row) over the members whose K is a number (0 = none)
inline void rep_decode(const uint32_t* rows, const float* gaps, const uint32_t* n, const uint64_t* reach_word, uint32_t C, uint32_t m,
                       const IdMap& map, uint64_t* picks, float* gap, uint32_t* n_picked, float* reach, uint64_t totals_out[3]) {
    uint64_t groups = 0, made = 0, rounds = 0;
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t k = n[c] < m ? n[c] : m;
        for (uint32_t j = 0; j < m; ++j) {
            const size_t at = (size_t)c * m + j;
            const bool has = j < k && rows[at] != REP_NO_ROW;
            if (picks) picks[at] = has ? id_of_local(map, rows[at]) : MI_KNN_NO_ID;
            if (gap) gap[at] = (has && j > 0) ? gaps[at] : INFINITY;
        }
        if (n_picked) n_picked[c] = k;
        if (reach) reach[c] = reach_word[c] != REP_SLOT_EMPTY ? summary_dist_of(rep_word_key(reach_word[c])) : INFINITY;
        groups += k != 0;
        made += k;
        if (k > rounds) rounds = k;
    }
    totals_out[0] = groups; totals_out[1] = made; totals_out[2] = rounds;
}

// what a table without rows answers: C empty groups
inline void rep_pad(uint32_t C, uint32_t m, uint64_t* picks, float* gap, uint32_t* n_picked, float* reach, uint64_t* totals) {
    for (size_t at = 0; at < (size_t)C * m; ++at) {
        if (picks) picks[at] = MI_KNN_NO_ID;
        if (gap) gap[at] = INFINITY;
    }
    for (uint32_t c = 0; c < C; ++c) {
        if (n_picked) n_picked[c] = 0;
        if (reach) reach[c] = INFINITY;
    }
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
}

}  // namespace mi
