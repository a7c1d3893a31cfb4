// The host-only pieces of mi_knn_search_ordered and mi_knn_stamp_histogram (image_search_amd/csrc/ordered_host.h) as a
// stand-alone program: the argument rules and their order, the order key at the 64-bit extremes in both directions, the cursor
// comparison inside a group of equal stamps, the cursor of a shard against a brute-force count over the block-cyclic placement,
// the edge rule, the bin of a stamp, the record's layout and the merge of the shards' lists.  Built with
// -fsanitize=address,undefined (tests/test_ordered_host.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_search_amd/csrc/ordered_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static mi_knn_where everything() { return mi_knn_where{0, 0, 0, INT64_MIN, INT64_MAX, 0, 0}; }

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    const float v[4] = {0, 0, 0, 0};
    mi_knn_where w = everything();
    const float inf = INFINITY;

    EXPECT(ordered_check_args(&t, v, 1, inf, nullptr, 0, &o, &o, &why) == MI_OK);
    EXPECT(ordered_check_args(&t, v, 4096, 0.5f, &w, MI_KNN_ORDER_DESC | MI_KNN_ORDER_AFTER, &o, &o, &why) == MI_OK);
    EXPECT(ordered_check_args(&t, v, 10, -0.5f, &w, 0, &o, &o, &why) == MI_OK);   // a negative bound is a bound
    EXPECT(ordered_check_args(nullptr, v, 1, inf, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID && why[0] != '\0');
    EXPECT(ordered_check_args(&t, nullptr, 1, inf, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_args(&t, v, 1, inf, nullptr, 0, nullptr, &o, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_args(&t, v, 1, inf, nullptr, 0, &o, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_args(&t, v, 1, NAN, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID && std::strstr(why, "NaN"));
    EXPECT(ordered_check_args(&t, v, 0, inf, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_args(&t, v, 4097, inf, nullptr, 0, &o, &o, &why) == MI_ERR_UNSUPPORTED);
    for (uint32_t bit = 2; bit < 32; ++bit) {   // every unknown flag, alone and beside the known ones
        EXPECT(ordered_check_args(&t, v, 1, inf, nullptr, 1u << bit, &o, &o, &why) == MI_ERR_INVALID);
        EXPECT(ordered_check_args(&t, v, 1, inf, nullptr, (1u << bit) | 3u, &o, &o, &why) == MI_ERR_INVALID && why[0] != '\0');
    }
    w.flags = 2;   // a bad predicate: where_host.h's rule
    EXPECT(ordered_check_args(&t, v, 1, inf, &w, 0, &o, &o, &why) == MI_ERR_INVALID);
    // the order: the bound before the flags before k
    EXPECT(ordered_check_args(&t, v, 0, NAN, nullptr, 4, &o, &o, &why) == MI_ERR_INVALID && std::strstr(why, "NaN"));
    EXPECT(ordered_check_args(&t, v, 4097, inf, nullptr, 4, &o, &o, &why) == MI_ERR_INVALID);
    w = everything();

    const int64_t e3[3] = {-5, 0, 7}, same[2] = {1, 1}, down[2] = {2, 1};
    uint64_t hist[4];
    EXPECT(ordered_check_hist_args(&t, v, inf, nullptr, e3, 3, hist, &why) == MI_OK);
    EXPECT(ordered_check_hist_args(&t, v, inf, &w, e3, 1, hist, &why) == MI_OK);
    EXPECT(ordered_check_hist_args(nullptr, v, inf, nullptr, e3, 3, hist, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_hist_args(&t, nullptr, inf, nullptr, e3, 3, hist, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_hist_args(&t, v, inf, nullptr, e3, 3, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_hist_args(&t, v, NAN, nullptr, e3, 3, hist, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_hist_args(&t, v, inf, nullptr, nullptr, 3, hist, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_hist_args(&t, v, inf, nullptr, e3, 0, hist, &why) == MI_ERR_INVALID);
    EXPECT(ordered_check_hist_args(&t, v, inf, nullptr, same, 2, hist, &why) == MI_ERR_INVALID && std::strstr(why, "ascending"));
    EXPECT(ordered_check_hist_args(&t, v, inf, nullptr, down, 2, hist, &why) == MI_ERR_INVALID);
    std::vector<int64_t> many(4097);
    for (size_t i = 0; i < many.size(); ++i) many[i] = (int64_t)i - 2000;
    EXPECT(ordered_edges_ok(many.data(), 4096, &why));
    EXPECT(!ordered_edges_ok(many.data(), 4097, &why));
    const int64_t ends[2] = {INT64_MIN, INT64_MAX};
    EXPECT(ordered_edges_ok(ends, 2, &why));
}

static void okey() {
    const int64_t s[5] = {INT64_MIN, -1, 0, 1, INT64_MAX};
    for (int i = 0; i + 1 < 5; ++i) {
        EXPECT(ordered_okey(s[i], false) < ordered_okey(s[i + 1], false));   // the unsigned order is the signed order ...
        EXPECT(ordered_okey(s[i], true) > ordered_okey(s[i + 1], true));     // ... and its reverse
    }
    EXPECT(ordered_okey(INT64_MIN, false) == 0 && ordered_okey(INT64_MAX, false) == UINT64_MAX);
    EXPECT(ordered_okey(INT64_MIN, true) == UINT64_MAX && ordered_okey(INT64_MAX, true) == 0);
    EXPECT(ordered_okey(0, false) == 0x8000000000000000ull);
    for (int i = 0; i < 5; ++i)
        for (int desc = 0; desc < 2; ++desc) EXPECT(ordered_stamp_of(ordered_okey(s[i], desc != 0), desc != 0) == s[i]);
}

static void cursor() {
    const IdMap plain{100, 0, 0, 0};   // 50 rows
    OrderedCursor c;
    EXPECT(ordered_cursor(plain, 50, 0, 7, 12345, &c) && c.on == 0 && c.desc == 0);              // no flag: after_* are not looked at
    EXPECT(ordered_past(c, 0, 0));
    EXPECT(ordered_cursor(plain, 50, MI_KNN_ORDER_DESC, 7, 12345, &c) && c.on == 0 && c.desc == 1);
    EXPECT(!ordered_cursor(plain, 50, MI_KNN_ORDER_AFTER, 7, 99, &c));                            // below the base
    EXPECT(!ordered_cursor(plain, 50, MI_KNN_ORDER_AFTER, 7, 150, &c));                           // past the last row
    EXPECT(!ordered_cursor(plain, 50, MI_KNN_ORDER_AFTER, 7, MI_KNN_NO_ID, &c));
    EXPECT(ordered_cursor(plain, 50, MI_KNN_ORDER_AFTER, 7, 110, &c) && c.on == 1 && c.first_row == 11 && c.okey == ordered_okey(7, false));
    // inside the group of stamp 7: rows up to the cursor's are behind it, the next one is past it; other stamps by their order
    EXPECT(!ordered_past(c, ordered_okey(7, false), 0) && !ordered_past(c, ordered_okey(7, false), 10));
    EXPECT(ordered_past(c, ordered_okey(7, false), 11) && ordered_past(c, ordered_okey(8, false), 0));
    EXPECT(!ordered_past(c, ordered_okey(6, false), 49) && !ordered_past(c, ordered_okey(-8, false), 49));
    EXPECT(ordered_cursor(plain, 50, MI_KNN_ORDER_AFTER | MI_KNN_ORDER_DESC, 7, 149, &c) && c.first_row == 50 && c.desc == 1);
    EXPECT(ordered_past(c, ordered_okey(6, true), 0) && !ordered_past(c, ordered_okey(8, true), 49));   // descending: smaller stamps follow
    EXPECT(!ordered_past(c, ordered_okey(7, true), 49));
    // the extremes as the cursor's stamp
    EXPECT(ordered_cursor(plain, 50, MI_KNN_ORDER_AFTER, INT64_MAX, 100, &c) && c.okey == UINT64_MAX);
    EXPECT(ordered_past(c, UINT64_MAX, 1) && !ordered_past(c, UINT64_MAX, 0) && !ordered_past(c, UINT64_MAX - 1, 49));
    // a shard of a block-cyclic table: the cursor's own row
    const IdMap shard{0, 8, 3, 1};   // 40 rows; blocks of 8 rows over 3 shards, this is shard 1: global rows 8..15, 32..39, ...
    EXPECT(ordered_cursor(shard, 40, MI_KNN_ORDER_AFTER, 0, 33, &c) && c.first_row == 10);
    EXPECT(!ordered_cursor(shard, 40, MI_KNN_ORDER_AFTER, 0, 16, &c));   // lives on shard 2
}

static void shard_cursor() {
    // brute force over the placement: global row r lives in block r / block, on shard (r / block) % n
    for (uint32_t block : {1u, 4u, 7u})
        for (uint32_t n : {1u, 3u, 8u})
            for (uint64_t after = 0; after < 100; ++after)
                for (uint32_t s = 0; s < n; ++s) {
                    uint64_t below = 0;
                    for (uint64_t r = 0; r <= after; ++r) below += (r / block) % n == s;
                    const OrderedCursor c = ordered_cursor_shard(block, n, s, MI_KNN_ORDER_AFTER | MI_KNN_ORDER_DESC, -3, after);
                    EXPECT(c.on == 1 && c.desc == 1 && c.first_row == below && c.okey == ordered_okey(-3, true));
                }
    const OrderedCursor c = ordered_cursor_shard(4, 3, 1, MI_KNN_ORDER_DESC, 5, 77);
    EXPECT(c.on == 0 && c.desc == 1);
}

static void bins() {
    const int64_t e[4] = {INT64_MIN + 1, -5, 0, 100};
    EXPECT(ordered_bin(e, 4, INT64_MIN) == 0 && ordered_bin(e, 4, INT64_MIN + 1) == 1);
    EXPECT(ordered_bin(e, 4, -6) == 1 && ordered_bin(e, 4, -5) == 2 && ordered_bin(e, 4, -1) == 2);   // an edge equal to a stamp counts
    EXPECT(ordered_bin(e, 4, 0) == 3 && ordered_bin(e, 4, 99) == 3 && ordered_bin(e, 4, 100) == 4 && ordered_bin(e, 4, INT64_MAX) == 4);
    EXPECT(ordered_bin(e, 1, INT64_MIN) == 0 && ordered_bin(e, 1, 0) == 1);
}

static void record_and_merge() {
    const uint32_t k = 3;
    const OrderedRecord r = ordered_record(k);
    EXPECT(r.idx == 0 && r.counts == 24 && r.stamps == 56 && r.dist == 80 && r.bytes == 92);
    std::vector<unsigned char> rec(r.bytes);
    const uint64_t idx[3] = {5, 6, MI_KNN_NO_ID}, counts[4] = {1, 2, 3, 4};   // the device's order: {before, within, beyond, nan}
    const int64_t stamps[3] = {-1, 9, 0};
    const float dist[3] = {0.5f, 0.25f, INFINITY};
    std::memcpy(rec.data() + r.idx, idx, sizeof idx);
    std::memcpy(rec.data() + r.counts, counts, sizeof counts);
    std::memcpy(rec.data() + r.stamps, stamps, sizeof stamps);
    std::memcpy(rec.data() + r.dist, dist, sizeof dist);
    uint64_t o_idx[3], o_counts[4];
    int64_t o_stamps[3];
    float o_dist[3];
    ordered_unpack(rec.data(), k, o_idx, o_dist, o_stamps, o_counts);
    EXPECT(!std::memcmp(o_idx, idx, sizeof idx) && !std::memcmp(o_stamps, stamps, sizeof stamps) && !std::memcmp(o_dist, dist, sizeof dist));
    EXPECT(o_counts[0] == 2 && o_counts[1] == 1 && o_counts[2] == 3 && o_counts[3] == 4);
    ordered_unpack(rec.data(), k, o_idx, o_dist, nullptr, nullptr);
    ordered_pad(k, o_idx, o_dist, o_stamps, o_counts);
    EXPECT(o_idx[0] == MI_KNN_NO_ID && o_idx[2] == MI_KNN_NO_ID && std::isinf(o_dist[1]) && o_stamps[2] == 0 && o_counts[0] == 0 && o_counts[3] == 0);
    ordered_pad(k, o_idx, o_dist, nullptr, nullptr);

    // three lists of k = 3, each in the result order; equal stamps break by id across lists
    const uint64_t NO = MI_KNN_NO_ID;
    const uint64_t l_idx[9] = {4, 1, NO, 2, 7, 9, NO, NO, NO};
    const int64_t l_st[9] = {-5, 3, 0, -5, 3, 3, 0, 0, 0};
    const float l_d[9] = {0.4f, 0.1f, INFINITY, 0.2f, 0.7f, 0.9f, INFINITY, INFINITY, INFINITY};
    uint64_t m_idx[3];
    int64_t m_st[3];
    float m_d[3];
    ordered_merge(l_idx, l_d, l_st, 3, 3, false, m_idx, m_d, m_st);
    EXPECT(m_idx[0] == 2 && m_idx[1] == 4 && m_idx[2] == 1 && m_st[0] == -5 && m_st[2] == 3 && m_d[0] == 0.2f && m_d[2] == 0.1f);
    // descending lists of the same rows
    const uint64_t d_idx[9] = {1, 4, NO, 7, 9, 2, NO, NO, NO};
    const int64_t d_st[9] = {3, -5, 0, 3, 3, -5, 0, 0, 0};
    ordered_merge(d_idx, l_d, d_st, 3, 3, true, m_idx, m_d, nullptr);
    EXPECT(m_idx[0] == 1 && m_idx[1] == 7 && m_idx[2] == 9);
    // fewer hits than k: padding behind
    const uint64_t s_idx[4] = {3, NO, NO, NO};
    const int64_t s_st[4] = {INT64_MIN, 0, 0, 0};
    const float s_d[4] = {0.5f, INFINITY, INFINITY, INFINITY};
    uint64_t p_idx[2];
    int64_t p_st[2];
    float p_d[2];
    ordered_merge(s_idx, s_d, s_st, 2, 2, false, p_idx, p_d, p_st);
    EXPECT(p_idx[0] == 3 && p_st[0] == INT64_MIN && p_idx[1] == NO && std::isinf(p_d[1]) && p_st[1] == 0);
}

int main() {
    args();
    okey();
    cursor();
    shard_cursor();
    bins();
    record_and_merge();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
