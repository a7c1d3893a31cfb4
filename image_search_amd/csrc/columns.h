// columns.h — one value per row of a table beside its vector: the group id, the tags, the stamp (handles.h).  A column exists
// from its first set call on.  Its device array is sized by the table's capacity (knn.hip: fit) and holds the default in every
// row nobody set; its host copy covers the rows it has been told about (columns_host.h: the rows beyond read as the default).
#pragma once
#include <cstring>
#include <vector>

#include "columns_host.h"
#include "device_mem.h"

namespace mi {

template <class T>
struct RowColumn : DevArray<T> {
    std::vector<T> host;
    const int fill;   // the default, as the byte the device array is filled with: 0xFF = no group, 0 = no tag / stamp 0
    explicit RowColumn(int fill_byte) : fill(fill_byte) {}
    T def() const {
        T v;
        std::memset(&v, fill, sizeof v);
        return v;
    }
    T get(size_t row) const { return column_get(host, row, def()); }
    T& slot(size_t rows, size_t row) { return column_slot(host, rows, def(), row); }   // rows: the table's
    // the rows from `rows` on are forgotten (a later append reuses them, with the default): the device tail refilled on s —
    // nothing in flight may use the column, and the caller waits for s — and the host copy cut
    void truncate(size_t rows, hipStream_t s) {
        if (this->p && rows < this->cap) HIP_CHECK(hipMemsetAsync(this->p + rows, fill, (this->cap - rows) * sizeof(T), s));
        column_truncate(host, rows);
    }
};

}  // namespace mi
