// table_csv_row.h -- a row of a typed table as text: the cells and the end of the line as table_csv.hip's row printer writes
// them, and the whole row a cell at a time for the host form (ysmr_table_format_devicelike) and tests/table_plan_check.cc.
// Plain C++ behind YSMR_HD, one text for the kernel and the host.
#pragma once
#include "fmt.h"
#include "table_csv_plan.h"

namespace tablep {

// a cell of one of the four integer types, straight into its place
YSMR_FMT_HD char *put_int_cell(char *q, int type, const void *data, long long row)
{
    if (type == COL_U32) return ysmr_fmt::put_dec32(q, ((const uint32_t *)data)[row]);
    if (type == COL_I64) return ysmr_fmt::put_int64(q, ((const int64_t *)data)[row]);
    const int32_t v = type == COL_I32 ? ((const int32_t *)data)[row] : (int32_t)((const int8_t *)data)[row];
    if (v < 0) *q++ = '-';
    return ysmr_fmt::put_dec32(q, v < 0 ? 0u - (uint32_t)v : (uint32_t)v);
}

// [line, q) holds the fields, a ',' behind each: the last becomes the '\n'.  A NaN that is its line's only field would leave the
// line empty, and to_csv (the csv module) writes "" there.  Returns the end.
YSMR_FMT_HD char *end_line(char *line, char *q)
{
    if (q - line == 1) { line[0] = '"'; line[1] = '"'; q = line + 3; }
    q[-1] = '\n';
    return q;
}

// HOST form: row `row` of the columns at p; at most row_bytes of row_of() are written.  *wide counts its wide cells.
YSMR_HD inline char *put_row(char *p, int n_columns, const int32_t *types, const void *const *data, long long row, long long *wide)
{
    char *const line = p;
    for (int c = 0; c < n_columns; ++c) {
        if (types[c] == COL_F64) {
            const double v = ((const double *)data[c])[row];
            *wide += ysmr_fmt::is_wide_cell(v) ? 1 : 0;
            p = ysmr_fmt::put_f64_field(p, v);
        } else p = put_int_cell(p, types[c], data[c], row);
        *p++ = ',';
    }
    return end_line(line, p);
}

}  // namespace tablep
