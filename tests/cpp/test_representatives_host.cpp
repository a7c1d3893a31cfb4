// The host-only pieces of mi_knn_representatives (image_search_amd/csrc/representatives_host.h) as a stand-alone program: the
// argument rules, the 64-bit word a group's candidates fold into, the min_gap window on keys, the translation of `start`, how
// the per-group arrays turn into ids and distances, and the padding of an empty table.  Built with
// -fsanitize=address,undefined (tests/test_representatives_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_search_amd/csrc/representatives_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static float float_of(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

static void args() {
    const char* why = nullptr;
    int t = 0;
    EXPECT(rep_check_args(&t, 1, 1, -INFINITY, &why) == MI_OK && why[0] == '\0');
    EXPECT(rep_check_args(&t, 65536, 64, 0.0f, &why) == MI_OK);          // C * m = 2^22 exactly
    EXPECT(rep_check_args(&t, 1024, 4096, INFINITY, &why) == MI_OK);
    EXPECT(rep_check_args(nullptr, 4, 4, 0.0f, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(rep_check_args(&t, 0, 4, 0.0f, &why) == MI_ERR_INVALID && std::strstr(why, "C must be"));
    EXPECT(rep_check_args(&t, 4, 0, 0.0f, &why) == MI_ERR_INVALID && std::strstr(why, "m must be"));
    EXPECT(rep_check_args(&t, 4, 4, NAN, &why) == MI_ERR_INVALID && std::strstr(why, "NaN"));
    EXPECT(rep_check_args(&t, 65537, 1, 0.0f, &why) == MI_ERR_UNSUPPORTED && std::strstr(why, "65536"));
    EXPECT(rep_check_args(&t, 1, 4097, 0.0f, &why) == MI_ERR_UNSUPPORTED && std::strstr(why, "4096"));
    EXPECT(rep_check_args(&t, 65536, 65, 0.0f, &why) == MI_ERR_UNSUPPORTED && std::strstr(why, "2^22"));
    EXPECT(rep_check_args(&t, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, &why) == MI_ERR_UNSUPPORTED);
    EXPECT(rep_check_args(nullptr, 0, 0, NAN, &why) == MI_ERR_INVALID && std::strstr(why, "null"));   // the handle first
    EXPECT(rep_check_args(&t, 0, 4097, 0.0f, &why) == MI_ERR_INVALID);                                 // a zero before a limit
    EXPECT(rep_check_args(&t, 65537, 4, NAN, &why) == MI_ERR_INVALID);                                 // NaN before a limit
}

static void words() {
    // the largest key wins; among equal keys the LOWEST row; every real word is above the empty slot
    const uint32_t k1 = summary_key_of(0.25f), k2 = summary_key_of(0.5f);
    EXPECT(rep_word(k2, 900) > rep_word(k1, 3));
    EXPECT(rep_word(k1, 3) > rep_word(k1, 4) && rep_word(k1, 0) > rep_word(k1, 0xFFFFFFFEu));
    EXPECT(rep_word(summary_key_of(-INFINITY), 0xFFFFFFFEu) > REP_SLOT_EMPTY);
    EXPECT(summary_key_of(-INFINITY) == 0x007FFFFFu);                    // the smallest key a number has: never 0
    for (uint32_t row : {0u, 1u, 511u, 0x7FFFFFFFu, 0xFFFFFFFEu}) {
        const uint64_t w = rep_word(k2, row);
        EXPECT(rep_word_key(w) == k2 && rep_word_row(w) == row);
    }
    EXPECT(rep_word(summary_key_of(0.0f), 7) > rep_word(summary_key_of(-0.0f), 2));    // -0 sorts before +0
}

static void window() {
    const uint64_t at_half = rep_word(summary_key_of(0.5f), 11);
    const float below = std::nextafterf(0.5f, 0.0f), above = std::nextafterf(0.5f, 1.0f);
    RepWindow w = rep_window(0.5f);
    EXPECT(w.bounded == 1 && !rep_takes(at_half, w.key, w.bounded));     // a pick is made only ABOVE the bound
    w = rep_window(below);
    EXPECT(rep_takes(at_half, w.key, w.bounded));
    w = rep_window(above);
    EXPECT(!rep_takes(at_half, w.key, w.bounded));
    w = rep_window(-INFINITY);
    EXPECT(w.bounded == 0 && rep_takes(at_half, w.key, w.bounded) && rep_takes(rep_word(summary_key_of(-INFINITY), 0), w.key, w.bounded));
    EXPECT(!rep_takes(REP_SLOT_EMPTY, w.key, w.bounded));                // no candidate is no pick, bound or not
    w = rep_window(INFINITY);
    EXPECT(w.bounded == 1 && !rep_takes(rep_word(summary_key_of(INFINITY), 0), w.key, w.bounded) && !rep_takes(at_half, w.key, w.bounded));
    w = rep_window(-0.0f);
    EXPECT(rep_takes(rep_word(summary_key_of(0.0f), 1), w.key, w.bounded) && !rep_takes(rep_word(summary_key_of(-0.0f), 1), w.key, w.bounded));
    w = rep_window(0.0f);
    EXPECT(!rep_takes(rep_word(summary_key_of(0.0f), 1), w.key, w.bounded));
    EXPECT(rep_takes(rep_word(summary_key_of(float_of(1u)), 1), w.key, w.bounded));    // the smallest denormal lies above 0
}

static void starts() {
    const IdMap plain{1000, 0, 0, 0};
    const uint64_t ids[5] = {1000, 1009, 1010, 999, 0xFFFFFFFFFFFFFFFFull};
    uint32_t out[5] = {7, 7, 7, 7, 7};
    rep_start_rows(plain, 10, ids, 5, out);
    EXPECT(out[0] == 0 && out[1] == 9 && out[2] == REP_NO_ROW && out[3] == REP_NO_ROW && out[4] == REP_NO_ROW);
    const IdMap shard{0, 4, 2, 1};                                       // rank 1 of 2, blocks of 4: ids 4..7, 12..15, ...
    const uint64_t sids[4] = {4, 13, 3, 8};
    rep_start_rows(shard, 8, sids, 4, out);
    EXPECT(out[0] == 0 && out[1] == 5 && out[2] == REP_NO_ROW && out[3] == REP_NO_ROW);
}

static void decode() {
    const uint32_t C = 3, m = 3;
    const IdMap map{500, 0, 0, 0};
    const uint32_t rows[C * m] = {4, 9, REP_NO_ROW, REP_NO_ROW, REP_NO_ROW, REP_NO_ROW, 2, 1, 0};
    const float gaps[C * m] = {INFINITY, 0.75f, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, 0.5f, -0.0f};
    const uint32_t n[C] = {2, 0, 3};
    const uint64_t reach_word[C] = {rep_word(summary_key_of(0.125f), 6), REP_SLOT_EMPTY, rep_word(summary_key_of(-0.0f), 0)};
    std::vector<uint64_t> picks(C * m, 1);
    std::vector<float> gap(C * m, -7.0f), reach(C, -7.0f);
    std::vector<uint32_t> n_picked(C, 7);
    uint64_t sums[3] = {9, 9, 9};
    rep_decode(rows, gaps, n, reach_word, C, m, map, picks.data(), gap.data(), n_picked.data(), reach.data(), sums);
    EXPECT(picks[0] == 504 && picks[1] == 509 && picks[2] == MI_KNN_NO_ID);
    EXPECT(picks[3] == MI_KNN_NO_ID && picks[4] == MI_KNN_NO_ID && picks[5] == MI_KNN_NO_ID);
    EXPECT(picks[6] == 502 && picks[7] == 501 && picks[8] == 500);
    EXPECT(std::isinf(gap[0]) && gap[1] == 0.75f && std::isinf(gap[2]) && std::isinf(gap[4]) && gap[7] == 0.5f);
    EXPECT(bits_of(gap[8]) == 0x80000000u);                              // the bits, not the value
    EXPECT(n_picked[0] == 2 && n_picked[1] == 0 && n_picked[2] == 3);
    EXPECT(reach[0] == 0.125f && std::isinf(reach[1]) && reach[1] > 0 && bits_of(reach[2]) == 0x80000000u);
    EXPECT(sums[0] == 2 && sums[1] == 5 && sums[2] == 3);
    // every output may be null
    rep_decode(rows, gaps, n, reach_word, C, m, map, nullptr, nullptr, nullptr, nullptr, sums);
    EXPECT(sums[0] == 2 && sums[1] == 5 && sums[2] == 3);
}

static void pad() {
    const uint32_t C = 2, m = 3;
    std::vector<uint64_t> picks(C * m, 1), totals(4, 9);
    std::vector<float> gap(C * m, -7.0f), reach(C, -7.0f);
    std::vector<uint32_t> n_picked(C, 7);
    rep_pad(C, m, picks.data(), gap.data(), n_picked.data(), reach.data(), totals.data());
    for (uint32_t i = 0; i < C * m; ++i) EXPECT(picks[i] == MI_KNN_NO_ID && std::isinf(gap[i]) && gap[i] > 0);
    for (uint32_t c = 0; c < C; ++c) EXPECT(n_picked[c] == 0 && std::isinf(reach[c]));
    EXPECT(totals[0] == 0 && totals[1] == 0 && totals[2] == 0 && totals[3] == 0);
    rep_pad(C, m, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int main() {
    args();
    words();
    window();
    starts();
    decode();
    pad();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
