// The host-only pieces of mi_knn_summarize (image_search_amd/csrc/summary_host.h) as a stand-alone program: the argument
// rules, the integer weight of a distance, the 32-bit distance keys, the words a workgroup reduces into and how the per-group
// slots turn into ids and distances, and the padding of an empty table.  Built with -fsanitize=address,undefined
// (tests/test_summary_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_search_amd/csrc/summary_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static float float_of(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

static void args() {
    const char* why = nullptr;
    int t = 0;
    EXPECT(summary_check_args(&t, 1, &why) == MI_OK && why[0] == '\0');
    EXPECT(summary_check_args(&t, 65536, &why) == MI_OK);
    EXPECT(summary_check_args(nullptr, 4, &why) == MI_ERR_INVALID && std::strstr(why, "null"));
    EXPECT(summary_check_args(&t, 0, &why) == MI_ERR_INVALID && std::strstr(why, "C must be"));
    EXPECT(summary_check_args(&t, 65537, &why) == MI_ERR_UNSUPPORTED && std::strstr(why, "65536"));
    EXPECT(summary_check_args(&t, 0xFFFFFFFFu, &why) == MI_ERR_UNSUPPORTED);
    EXPECT(summary_check_args(nullptr, 0, &why) == MI_ERR_INVALID && std::strstr(why, "null"));   // the handle first
}

static void weights() {
    EXPECT(summary_weight(0.0f) == 0 && summary_weight(-0.0f) == 0 && summary_weight(-1e-7f) == 0 && summary_weight(-INFINITY) == 0);
    EXPECT(summary_weight(1.0f) == (1u << 30) && summary_weight(0.5f) == (1u << 29) && summary_weight(0.25f) == (1u << 28));
    EXPECT(summary_weight(2.0f) == (1u << 31) && summary_weight(2.0000002f) == (1u << 31) && summary_weight(INFINITY) == (1u << 31));
    EXPECT(summary_weight(float_of(0x3F800001u)) == (1u << 30) + (1u << 7));   // 1 + 2^-23: the scaling is exact
    EXPECT(summary_weight(float_of(0x00000001u)) == 0);                        // a denormal truncates to 0
    EXPECT(summary_weight(float_of(0x3FFFFFFFu)) == 0x7FFFFF80u);              // the largest float below 2
    // 2^32 rows at the largest weight still fit the 64-bit sum
    EXPECT((uint64_t)summary_weight(2.0f) * 0xFFFFFFFFull < 0xFFFFFFFFFFFFFFFFull);
}

static void keys() {
    const float d[] = {-INFINITY, -1.5f, -0.0f, 0.0f, float_of(1u), 0.25f, 2.0f, INFINITY};
    for (size_t i = 0; i + 1 < sizeof d / sizeof d[0]; ++i) EXPECT(summary_key_of(d[i]) < summary_key_of(d[i + 1]));
    for (float x : d) EXPECT(bits_of(summary_dist_of(summary_key_of(x))) == bits_of(x));
    EXPECT(summary_key_of(NAN) == 0xFFFFFFFFu && summary_key_of(float_of(0xFFC00001u)) == 0xFFFFFFFFu);
    EXPECT(summary_key_of(INFINITY) < 0xFFFFFFFFu);
    const float back = summary_dist_of(0xFFFFFFFFu);
    EXPECT(back != back);
    EXPECT(summary_key_of(-INFINITY) != 0);   // no number has the key 0: the max slot's start value is free
    // the words: the min word prefers the lower row among equal keys, the max word too
    EXPECT(summary_min_word(5, 3) < summary_min_word(5, 4) && summary_min_word(5, 0xFFFFFFFEu) < summary_min_word(6, 0));
    EXPECT(summary_max_word(5, 3) > summary_max_word(5, 4) && summary_max_word(6, 0xFFFFFFFEu) > summary_max_word(5, 0));
    EXPECT(summary_max_word(summary_key_of(-INFINITY), 0xFFFFFFFEu) > SUMMARY_MAX_INIT);
    EXPECT(summary_min_word(0xFFFFFFFFu, 0xFFFFFFFEu) < SUMMARY_MIN_INIT);
}

static void decode() {
    const uint32_t C = 4;
    // group 0: rows 7 (0.25) and 9 (0.75); group 1: empty; group 2: one NaN member at row 2; group 3: rows 4, 5 at -0 / +0
    std::vector<uint64_t> slots(SUMMARY_PLANES * C);
    const uint32_t count[C] = {2, 0, 1, 2};
    slots[0] = summary_min_word(summary_key_of(0.25f), 7);
    slots[C + 0] = summary_max_word(summary_key_of(0.75f), 9);
    slots[2 * C + 0] = 2;
    slots[3 * C + 0] = (uint64_t)summary_weight(0.25f) + summary_weight(0.75f);
    slots[1] = SUMMARY_MIN_INIT; slots[C + 1] = SUMMARY_MAX_INIT;
    slots[2] = summary_min_word(summary_key_of(NAN), 2); slots[C + 2] = SUMMARY_MAX_INIT;
    slots[3] = summary_min_word(summary_key_of(-0.0f), 5);
    slots[C + 3] = summary_max_word(summary_key_of(0.0f), 4);
    slots[2 * C + 3] = 2;
    uint64_t cover[C], odd[C], measured[C], spread[C];
    float cover_dist[C], odd_dist[C];
    const IdMap plain{1000, 0, 0, 0};
    summary_decode(slots.data(), count, C, plain, cover, cover_dist, odd, odd_dist, measured, spread);
    EXPECT(cover[0] == 1007 && cover_dist[0] == 0.25f && odd[0] == 1009 && odd_dist[0] == 0.75f && measured[0] == 2);
    EXPECT(spread[0] == (1ull << 28) + (3ull << 28));
    EXPECT(cover[1] == MI_KNN_NO_ID && std::isinf(cover_dist[1]) && odd[1] == MI_KNN_NO_ID && std::isinf(odd_dist[1]));
    EXPECT(measured[1] == 0 && spread[1] == 0);
    EXPECT(cover[2] == 1002 && cover_dist[2] != cover_dist[2] && odd[2] == MI_KNN_NO_ID && std::isinf(odd_dist[2]) && measured[2] == 0);
    EXPECT(cover[3] == 1005 && bits_of(cover_dist[3]) == 0x80000000u && odd[3] == 1004 && bits_of(odd_dist[3]) == 0u);
    // a shard of a block-cyclic table: block 4, 3 shards, rank 1 — local row 5 is global row (1 * 3 + 1) * 4 + 1 = 17
    const IdMap cyc{0, 4, 3, 1};
    summary_decode(slots.data(), count, C, cyc, cover, nullptr, odd, nullptr, nullptr, nullptr);
    EXPECT(cover[3] == 17 && odd[3] == 16 && cover[0] == id_of_local(cyc, 7));
    // every output may be null
    summary_decode(slots.data(), count, C, plain, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    // the highest row a table can hold
    const uint64_t one[SUMMARY_PLANES] = {summary_min_word(summary_key_of(0.5f), 0xFFFFFFFEu),
                                          summary_max_word(summary_key_of(0.5f), 0xFFFFFFFEu), 1, summary_weight(0.5f)};
    summary_decode(one, count, 1, plain, cover, cover_dist, odd, odd_dist, nullptr, nullptr);
    EXPECT(cover[0] == 1000ull + 0xFFFFFFFEull && odd[0] == cover[0] && odd_dist[0] == 0.5f);
}

static void pad() {
    const uint32_t C = 3, dim = 4;
    std::vector<float> cent(C * dim, 7.0f), cd(C, 7.0f), od(C, 7.0f);
    std::vector<uint64_t> count(C, 7), cover(C, 7), odd(C, 7), measured(C, 7), spread(C, 7);
    uint64_t totals[4] = {7, 7, 7, 7};
    summary_pad(C, dim, cent.data(), count.data(), cover.data(), cd.data(), odd.data(), od.data(), measured.data(), spread.data(), totals);
    for (float v : cent) EXPECT(bits_of(v) == 0);
    for (uint32_t c = 0; c < C; ++c) {
        EXPECT(count[c] == 0 && cover[c] == MI_KNN_NO_ID && odd[c] == MI_KNN_NO_ID && measured[c] == 0 && spread[c] == 0);
        EXPECT(std::isinf(cd[c]) && cd[c] > 0 && std::isinf(od[c]) && od[c] > 0);
    }
    EXPECT(totals[0] == 0 && totals[1] == 0 && totals[2] == 0 && totals[3] == 0);
    summary_pad(C, dim, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int main() {
    args();
    weights();
    keys();
    decode();
    pad();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
