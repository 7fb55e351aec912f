// table_wide.h -- the wide cells of a table's float64 columns printed into their side slots, for the two row printers
// (table_csv.hip, where the kernels are, and xlsx.hip): the pre-pass, the prefix sum and the wide printer's launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace tablep {

// wide_incl [n_rows]: wide cells per row, then their inclusive sums; wide_temp: scan_words(n_rows) words; slots / slot_len:
// 24 bytes and a length per wide cell, in (row, column) order; *wide_cells_dev: their number.  n_rows > 0, a float64 column
// among the n_columns.  Asynchronous on st.
void launch_wide_cells(hipStream_t st, int n_columns, const void *const *data, const int32_t *types, long long n_rows,
                       uint32_t *wide_incl, uint32_t *wide_temp, char *slots, uint8_t *slot_len, uint32_t *wide_cells_dev);

}  // namespace tablep
