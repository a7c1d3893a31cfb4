// columns_host.h — the host copy of a per-row column (the group id, the tags, the stamps; RowColumn in columns.h): a vector
// that covers the rows it has been told about, every row beyond its end holding the column's default.  No HIP in here:
// tests/cpp/test_columns_host.cpp compiles this header alone and runs it under the sanitizers.
#pragma once
#include <cstddef>
#include <vector>

namespace mi {

// what `row` holds
template <class T>
inline T column_get(const std::vector<T>& col, size_t row, T def) {
    return row < col.size() ? col[row] : def;
}

// the entry of `row` (< rows) to write to; the column first covers the table's `rows`, the entries it gains hold the default
template <class T>
inline T& column_slot(std::vector<T>& col, size_t rows, T def, size_t row) {
    if (col.size() < rows) col.resize(rows, def);
    return col[row];
}

// the rows from `rows` on are forgotten (a column that ends before them stays as it is)
template <class T>
inline void column_truncate(std::vector<T>& col, size_t rows) {
    if (col.size() > rows) col.resize(rows);
}

// `dead`: rows that leave the table — ascending, once each.  Their entries leave, the others close up in order (a column
// shorter than the table stays shorter: the rows it was never told about hold the default).  Returns the entries that left.
template <class T, class I>
inline size_t compact_column(std::vector<T>& col, const std::vector<I>& dead) {
    size_t c = 0, w = 0;
    for (size_t o = 0; o < col.size(); ++o) {
        if (c < dead.size() && dead[c] == o) { ++c; continue; }
        col[w++] = col[o];
    }
    col.resize(w);
    return c;
}

}  // namespace mi
