// xlsx_row.h -- a row of a typed table as SpreadsheetML: <row r="N">, its cells and </row> as xlsx.hip's row printer writes
// them, and the whole row a cell at a time for the host form (ysmr_xlsx_sheet_devicelike) and tests/xlsx_plan_check.cc.
// Plain C++ behind YSMR_HD, one text for the kernel and the host.
//   <row r="7"><c r="A7" s="1"><v>5</v></c><c r="B7"><v>1.5</v></c><c r="D7"><v>-3</v></c></row>
// Every cell carries its reference (a column letter A .. Q, the sheet row in 1 .. 7 digits).  The index cell (style 1) holds
// the table's row number.  Integers are plain decimals, a float64 is fmt.h's text; a NaN cell is NOT WRITTEN (C7 above), so a
// row of only NaN cells is its <row>, its index cell and </row>.  An infinity -- the reader (csv_parse.h) never gives one --
// is written as the string cell <c r="B7" t="str"><v>inf</v></c>.
#pragma once
#include "fmt.h"
#include "table_csv_row.h"
#include "xlsx_plan.h"

namespace xlsxp {

template <int N>
YSMR_FMT_HD char *put_lit(char *q, const char (&text)[N])
{
#pragma unroll
    for (int i = 0; i < N - 1; ++i) q[i] = text[i];
    return q + (N - 1);
}

YSMR_FMT_HD bool is_nan(double v) { return (ysmr_fmt::bits_of(v) & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
YSMR_FMT_HD bool is_inf(double v) { return (ysmr_fmt::bits_of(v) & 0x7FFFFFFFFFFFFFFFull) == 0x7FF0000000000000ull; }

YSMR_FMT_HD char *row_open(char *q, uint32_t sheet_row)
{
    q = put_lit(q, "<row r=\"");
    q = ysmr_fmt::put_dec32(q, sheet_row);
    return put_lit(q, "\">");
}

YSMR_FMT_HD char *row_close(char *q) { return put_lit(q, "</row>"); }

// the cell of column A that holds the table's row number
YSMR_FMT_HD char *index_cell(char *q, uint32_t sheet_row, uint32_t index)
{
    q = put_lit(q, "<c r=\"A");
    q = ysmr_fmt::put_dec32(q, sheet_row);
    q = put_lit(q, "\" s=\"1\"><v>");
    q = ysmr_fmt::put_dec32(q, index);
    return put_lit(q, "</v></c>");
}

// <c r="B7"><v> of sheet column `column` (0: A); as_text: the value is a string
YSMR_FMT_HD char *cell_open(char *q, int column, uint32_t sheet_row, bool as_text)
{
    q = put_lit(q, "<c r=\"");
    *q++ = (char)('A' + column);
    q = ysmr_fmt::put_dec32(q, sheet_row);
    return as_text ? put_lit(q, "\" t=\"str\"><v>") : put_lit(q, "\"><v>");
}

YSMR_FMT_HD char *cell_close(char *q) { return put_lit(q, "</v></c>"); }

// HOST form: row `row` of the columns at p; at most row_bytes of row_of() are written.  *wide counts its wide cells.
YSMR_HD inline char *put_row(char *p, int n_columns, const int32_t *types, const void *const *data, long long row, long long first_row,
                             bool with_index, long long *wide)
{
    const uint32_t sheet_row = (uint32_t)(first_row + row);
    p = row_open(p, sheet_row);
    if (with_index) p = index_cell(p, sheet_row, (uint32_t)row);
    for (int c = 0; c < n_columns; ++c) {
        const int column = c + (with_index ? 1 : 0);
        if (types[c] == tablep::COL_F64) {
            const double v = ((const double *)data[c])[row];
            if (is_nan(v)) continue;
            *wide += ysmr_fmt::is_wide_cell(v) ? 1 : 0;
            p = cell_open(p, column, sheet_row, is_inf(v));
            p = ysmr_fmt::put_f64_field(p, v);
        } else {
            p = cell_open(p, column, sheet_row, false);
            p = tablep::put_int_cell(p, types[c], data[c], row);
        }
        p = cell_close(p);
    }
    return row_close(p);
}

}  // namespace xlsxp
