// Stand-alone host test of image_search_amd/csrc/columns_host.h: the host copy of a per-row column — read with the default
// beyond the end, write that first extends to the table's rows, truncation, and the compaction by a list of deleted rows of
// either integer width — against brute-force restatements.  Built with the address and undefined-behaviour sanitizers by
// tests/test_columns_host.py; needs neither the library nor a GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../image_search_amd/csrc/columns_host.h"

using namespace mi;

static int failures = 0;
#define CHECK(c, ...)                                                   \
    do {                                                                \
        if (!(c)) {                                                     \
            ++failures;                                                 \
            std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c);  \
            std::printf(__VA_ARGS__);                                   \
            std::printf("\n");                                          \
        }                                                               \
    } while (0)

static const size_t LENGTHS[] = {0, 1, 63, 64, 65, 200};

// entry r of the column under test: never the default, different for every row
template <class T>
static T value_of(size_t r) { return (T)(1000 + 7 * r); }

template <class T>
static std::vector<T> column_of(size_t len) {
    std::vector<T> col(len);
    for (size_t r = 0; r < len; ++r) col[r] = value_of<T>(r);
    return col;
}

template <class T>
static void test_get(T def, const char* nm) {
    for (size_t len : LENGTHS) {
        const std::vector<T> col = column_of<T>(len);
        for (size_t r = 0; r < len + 70; ++r)   // ... the end itself (r == len) and far beyond it
            CHECK(column_get(col, r, def) == (r < len ? value_of<T>(r) : def), "%s len %zu: row %zu", nm, len, r);
    }
}

// one write to `row` of a table of `rows`: the column covers max(len, rows) afterwards, the entries it gained hold the default,
// the ones it had are untouched, and `row` holds what was written
template <class T>
static void test_slot(T def, const char* nm) {
    for (size_t len : LENGTHS)
        for (size_t rows : {len, len + 1, len + 64, (size_t)300}) {
            if (rows == 0) continue;
            for (size_t row : {(size_t)0, rows / 2, rows - 1}) {
                std::vector<T> col = column_of<T>(len);
                column_slot(col, rows, def, row) = (T)5;
                CHECK(col.size() == (len > rows ? len : rows), "%s len %zu rows %zu: size %zu", nm, len, rows, col.size());
                bool same = true;
                for (size_t r = 0; r < col.size(); ++r) same = same && col[r] == (r == row ? (T)5 : r < len ? value_of<T>(r) : def);
                CHECK(same, "%s len %zu rows %zu row %zu: contents", nm, len, rows, row);
            }
        }
    // a column longer than the table (rows were truncated away beneath a caller that still holds the length) is not cut
    std::vector<T> col = column_of<T>(65);
    column_slot(col, 10, def, 3) = (T)5;
    CHECK(col.size() == 65 && col[3] == (T)5 && col[64] == value_of<T>(64), "%s: a write must not shorten", nm);
}

template <class T>
static void test_truncate(const char* nm) {
    for (size_t len : LENGTHS)
        for (size_t rows : {(size_t)0, len / 2, len, len + 1, len + 64}) {
            std::vector<T> col = column_of<T>(len);
            column_truncate(col, rows);
            CHECK(col.size() == (rows < len ? rows : len), "%s len %zu to %zu: size %zu", nm, len, rows, col.size());
            bool same = true;
            for (size_t r = 0; r < col.size(); ++r) same = same && col[r] == value_of<T>(r);
            CHECK(same, "%s len %zu to %zu: contents", nm, len, rows);
        }
}

// the dead lists of a table of `rows`: none, the first row, the last row, every row, alternating rows
template <class I>
static std::vector<std::vector<I>> dead_lists(size_t rows) {
    std::vector<std::vector<I>> lists(5);
    if (rows) {
        lists[1].push_back(0);
        lists[2].push_back((I)(rows - 1));
    }
    for (size_t r = 0; r < rows; ++r) lists[3].push_back((I)r);
    for (size_t r = 0; r < rows; r += 2) lists[4].push_back((I)r);
    return lists;
}

// the table holds max(len, 1) + 10 rows: the column may be shorter than the table, and deleted rows may lie beyond its end
template <class T, class I>
static void test_compact(const char* nm) {
    for (size_t len : LENGTHS)
        for (size_t rows : {len, len + 10}) {
            const std::vector<std::vector<I>> lists = dead_lists<I>(rows);
            for (size_t which = 0; which < lists.size(); ++which) {
                const std::vector<I>& dead = lists[which];
                std::vector<char> is_dead(rows + 1, 0);
                for (I d : dead) is_dead[(size_t)d] = 1;
                std::vector<T> want;
                size_t left = 0;
                for (size_t r = 0; r < len; ++r) {
                    if (is_dead[r]) ++left;
                    else want.push_back(value_of<T>(r));
                }
                std::vector<T> col = column_of<T>(len);
                const size_t got = compact_column(col, dead);
                CHECK(got == left, "%s len %zu rows %zu list %zu: %zu entries left, want %zu", nm, len, rows, which, got, left);
                CHECK(col == want, "%s len %zu rows %zu list %zu: contents", nm, len, rows, which);
            }
        }
}

int main() {
    test_get<uint32_t>(0xFFFFFFFFu, "groups get");
    test_get<uint64_t>(0, "tags get");
    test_get<int64_t>(0, "stamps get");
    test_slot<uint32_t>(0xFFFFFFFFu, "groups set");
    test_slot<uint64_t>(0, "tags set");
    test_slot<int64_t>(0, "stamps set");
    test_truncate<uint32_t>("groups truncate");
    test_truncate<int64_t>("stamps truncate");
    test_compact<uint32_t, uint32_t>("groups by u32");
    test_compact<uint64_t, uint32_t>("tags by u32");
    test_compact<int64_t, uint32_t>("stamps by u32");
    test_compact<uint32_t, uint64_t>("groups by u64");
    test_compact<uint64_t, uint64_t>("tags by u64");
    test_compact<int64_t, uint64_t>("stamps by u64");
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
