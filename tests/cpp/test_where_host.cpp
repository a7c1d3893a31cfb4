// The host-only pieces of mi_knn_search_where and its kin (image_search_amd/csrc/where_host.h) as a stand-alone program: the
// argument rules (unknown flags, null pointers, the k limits and their order), the predicate on one row against hand cases
// (bit 63, signed bounds at the 64-bit extremes, the group flag with and without a column), the predicates known to match
// nothing, and the "where_chunk" rule.  Built with -fsanitize=address,undefined (tests/test_where_host.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image_search_amd/csrc/where_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static mi_knn_where everything() { return mi_knn_where{0, 0, 0, INT64_MIN, INT64_MAX, 0, 0}; }

static void args() {
    const char* why = nullptr;
    int t = 0, o = 0;
    const float v[4] = {0, 0, 0, 0};
    mi_knn_where w = everything();
    uint64_t count = 0;

    EXPECT(where_check_pred(&w, &why) == MI_OK);
    EXPECT(where_check_pred(nullptr, &why) == MI_ERR_INVALID && why[0] != '\0');
    w.flags = MI_KNN_WHERE_GROUP;
    EXPECT(where_check_pred(&w, &why) == MI_OK);
    for (uint32_t bit = 1; bit < 32; ++bit) {   // every other bit, alone and beside the known one
        w.flags = 1u << bit;
        EXPECT(where_check_pred(&w, &why) == MI_ERR_INVALID);
        w.flags |= MI_KNN_WHERE_GROUP;
        EXPECT(where_check_pred(&w, &why) == MI_ERR_INVALID && why[0] != '\0');
    }
    w = everything();

    EXPECT(where_check_rows_args(&t, &w, nullptr, 0, &count, &why) == MI_OK);
    EXPECT(where_check_rows_args(&t, &w, &o, 5, &count, &why) == MI_OK);
    EXPECT(where_check_rows_args(nullptr, &w, nullptr, 0, &count, &why) == MI_ERR_INVALID);
    EXPECT(where_check_rows_args(&t, nullptr, nullptr, 0, &count, &why) == MI_ERR_INVALID);
    EXPECT(where_check_rows_args(&t, &w, nullptr, 0, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(where_check_rows_args(&t, &w, nullptr, 5, &count, &why) == MI_ERR_INVALID);   // room promised, no array

    auto chk = [&](const void* tt, const void* q, uint32_t nq, uint32_t k, const mi_knn_where* ww, const void* idx, const void* dist) {
        return where_check_search_args(tt, q, nq, k, ww, idx, dist, &why);
    };
    EXPECT(chk(&t, v, 1, 1, &w, &o, &o) == MI_OK);
    EXPECT(chk(&t, v, 8, 4096, &w, &o, &o) == MI_OK);
    EXPECT(chk(&t, nullptr, 0, 10, &w, nullptr, nullptr) == MI_OK);                      // no query: no pointers needed
    EXPECT(chk(nullptr, v, 1, 1, &w, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, nullptr, 1, 1, &w, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 1, &w, nullptr, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 1, &w, &o, nullptr) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 1, nullptr, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 0, &w, &o, &o) == MI_ERR_INVALID);
    EXPECT(chk(&t, v, 1, 4097, &w, &o, &o) == MI_ERR_UNSUPPORTED);
    EXPECT(chk(&t, v, 1, 0xFFFFFFFFu, &w, &o, &o) == MI_ERR_UNSUPPORTED);
    w.flags = 2;
    EXPECT(chk(&t, v, 1, 4097, &w, &o, &o) == MI_ERR_INVALID);                           // the predicate is judged before k
    EXPECT(why && why[0] != '\0');
    w = everything();

    const uint64_t ids[1] = {0};
    EXPECT(where_check_attrs_args(&t, ids, 1, &why) == MI_OK);
    EXPECT(where_check_attrs_args(&t, nullptr, 0, &why) == MI_OK);
    EXPECT(where_check_attrs_args(nullptr, ids, 1, &why) == MI_ERR_INVALID);
    EXPECT(where_check_attrs_args(&t, nullptr, 1, &why) == MI_ERR_INVALID);
}

static void predicate() {
    const uint64_t B63 = 1ull << 63;
    mi_knn_where w = everything();
    EXPECT(where_row(w, 0, 0, false, 0) && where_row(w, ~0ull, INT64_MIN, false, 0) && where_row(w, B63, INT64_MAX, true, 9));
    w.all_of = 0b011;
    EXPECT(where_row(w, 0b011, 0, false, 0) && where_row(w, 0b111, 0, false, 0) && !where_row(w, 0b001, 0, false, 0) && !where_row(w, 0, 0, false, 0));
    w = everything();
    w.any_of = 0b110;
    EXPECT(where_row(w, 0b100, 0, false, 0) && where_row(w, 0b011, 0, false, 0) && !where_row(w, 0b001, 0, false, 0) && !where_row(w, 0, 0, false, 0));
    w = everything();
    w.none_of = 0b101;
    EXPECT(where_row(w, 0b010, 0, false, 0) && !where_row(w, 0b100, 0, false, 0) && !where_row(w, 0b111, 0, false, 0));
    w = everything();
    w.all_of = B63;
    EXPECT(where_row(w, B63, 0, false, 0) && where_row(w, ~0ull, 0, false, 0) && !where_row(w, B63 - 1, 0, false, 0));
    w.all_of = 0; w.none_of = B63;
    EXPECT(!where_row(w, B63, 0, false, 0) && where_row(w, B63 - 1, 0, false, 0));
    // signed bounds
    w = everything();
    w.stamp_hi = -1;
    EXPECT(where_row(w, 0, -1, false, 0) && where_row(w, 0, INT64_MIN, false, 0) && !where_row(w, 0, 0, false, 0) && !where_row(w, 0, INT64_MAX, false, 0));
    w = everything();
    w.stamp_lo = INT64_MAX;
    EXPECT(where_row(w, 0, INT64_MAX, false, 0) && !where_row(w, 0, INT64_MAX - 1, false, 0) && !where_row(w, 0, INT64_MIN, false, 0));
    w = everything();
    w.stamp_lo = w.stamp_hi = INT64_MIN;
    EXPECT(where_row(w, 0, INT64_MIN, false, 0) && !where_row(w, 0, INT64_MIN + 1, false, 0));
    w.stamp_lo = 1; w.stamp_hi = 0;
    EXPECT(!where_row(w, 0, 0, false, 0) && !where_row(w, 0, 1, false, 0));
    // the group flag
    w = everything();
    w.group = 3;
    EXPECT(where_row(w, 0, 0, true, 4));                                        // without the flag the group is not looked at
    w.flags = MI_KNN_WHERE_GROUP;
    EXPECT(where_row(w, 0, 0, true, 3) && !where_row(w, 0, 0, true, 4) && !where_row(w, 0, 0, true, MI_KNN_NO_GROUP));
    EXPECT(!where_row(w, 0, 0, false, 3));                                      // no column: nothing
    w.group = MI_KNN_NO_GROUP;
    EXPECT(where_row(w, 0, 0, true, MI_KNN_NO_GROUP) && !where_row(w, 0, 0, true, 0) && !where_row(w, 0, 0, false, MI_KNN_NO_GROUP));

    // what can be refused without looking at a row agrees with the row rule
    w = everything();
    EXPECT(!where_never(w, false) && !where_never(w, true));
    w.stamp_lo = 5; w.stamp_hi = 4;
    EXPECT(where_never(w, true));
    w = everything();
    w.all_of = 0b110; w.none_of = 0b100;
    EXPECT(where_never(w, true) && !where_row(w, 0b110, 0, true, 0) && !where_row(w, 0b010, 0, true, 0));
    w.none_of = 0b001;
    EXPECT(!where_never(w, true));
    w = everything();
    w.flags = MI_KNN_WHERE_GROUP;
    EXPECT(where_never(w, false) && !where_never(w, true));
}

static void chunks() {
    EXPECT(where_chunk_ok(0) && where_chunk_ok(64) && where_chunk_ok(256) && where_chunk_ok(4096) && where_chunk_ok(65536));
    EXPECT(!where_chunk_ok(-64) && !where_chunk_ok(1) && !where_chunk_ok(63) && !where_chunk_ok(100) && !where_chunk_ok(65600) && !where_chunk_ok(1 << 20));
    EXPECT(where_chunk_rows(0) == WHERE_CHUNK_DEFAULT && where_chunk_rows(64) == 64 && WHERE_CHUNK_DEFAULT % 64 == 0);
    EXPECT(where_chunks(0, 64) == 0 && where_chunks(1, 64) == 1 && where_chunks(64, 64) == 1 && where_chunks(65, 64) == 2);
    EXPECT(where_chunks(70000, 64) == 1094 && where_chunks(0xFFFFFFFFull, 64) == (1u << 26));
    EXPECT(where_chunks(10000000, WHERE_CHUNK_DEFAULT) == 2442);
}

int main() {
    args();
    predicate();
    chunks();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
