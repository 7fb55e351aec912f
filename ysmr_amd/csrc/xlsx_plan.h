// xlsx_plan.h -- the host-only part of xlsx.hip: the widths of a sheet's cells, the longest row of a set of column types, the
// geometry of the row printer, the bound of a sheet's XML and the layout of the workspace, with what they refuse.  Plain C++
// with no HIP in it, so that tests/xlsx_plan_check.cc compiles it alone, under the host sanitizers.  Column types, field
// widths, the side slots of wide cells and the scans' sizes are table_csv_plan.h's.
#pragma once
#include <cstddef>
#include <cstdint>

#include "table_csv_plan.h"

namespace xlsxp {

constexpr int MAX_COLUMNS = tablep::MAX_COLUMNS;
constexpr long long MAX_SHEET_ROW = 1048576;                 // the last row of a sheet
constexpr int ROW_DIGITS = 7;                                // ... and its digits
// <c r="Q1048576"><v> ... </v></c>: 6 + a letter + the row + 5, the value, 8
constexpr int CELL_OVERHEAD = 6 + 1 + ROW_DIGITS + 5 + 8;    // 27
// <c r="A1048576" s="1"><v>1048575</v></c>: the index cell, 6 + 1 + 7 + 11 + 7 + 8
constexpr int INDEX_CELL = 6 + 1 + ROW_DIGITS + 11 + ROW_DIGITS + 8;      // 40
// <row r="1048576"> ... </row>: 8 + 7 + 2, 6
constexpr int ROW_OVERHEAD = 8 + ROW_DIGITS + 2 + 6;         // 23
// (an infinity is <c r="Q1048576" t="str"><v>-inf</v></c>, 39 bytes: shorter than a float64 cell of 24 digits, 51)
static_assert(CELL_OVERHEAD + 8 + 4 <= CELL_OVERHEAD + tablep::FIELD_WIDTH[tablep::COL_F64], "an infinity's cell fits a float64 cell");

// ---- geometry (ysmr_xlsx_sheet_geometry reports it) --------------------------------------------------------------------------
constexpr int MAX_ROW_BYTES = ROW_OVERHEAD + INDEX_CELL + MAX_COLUMNS * (CELL_OVERHEAD + tablep::FIELD_WIDTH[tablep::COL_F64]);   // 879
constexpr int MAX_ROW_STRIDE = (MAX_ROW_BYTES + 3) / 4 * 4;                                                                        // 880
// a row per lane, one wave: the staging of the widest row (sixteen float64 columns behind the index) is 56320 bytes of dynamic
// LDS, which with the row offsets and a lane's digits stays inside the 64 KiB of a workgroup; two waves of such rows would not
constexpr int ROWS_PER_GROUP = 64;
constexpr int STAGED_BYTES = ROWS_PER_GROUP * MAX_ROW_STRIDE;
static_assert(STAGED_BYTES + 4096 <= 65536, "the staging of the widest row, the offsets and the digits fit a workgroup's LDS");
constexpr size_t MAX_TEXT = tablep::MAX_TEXT;               // byte offsets and counts are 32-bit numbers in the scans

using Plan = tablep::Plan;                                  // (its `suffix` area holds the sheet's end for the packing launch)

// table row 0 is sheet row first_row: false where a row would lie outside the sheet
inline bool rows_fit(long long n_rows, long long first_row)
{
    return n_rows >= 0 && first_row >= 1 && first_row <= MAX_SHEET_ROW && n_rows <= MAX_SHEET_ROW - first_row + 1;
}

inline int digits_of(long long v)
{
    int n = 1;
    for (; v >= 10; v /= 10) ++n;
    return n;
}

// The longest row of THIS table: cells of the declared types' widest values under the digits of its last sheet row and of its
// last row number (a sheet of 2^20 rows: MAX_ROW_BYTES with sixteen float64 columns).  false: a column count outside 1 .. 16,
// an unknown type, rows outside the sheet
inline bool row_of(int n_columns, const int32_t *types, bool with_index, long long n_rows, long long first_row, int &row_bytes, int &n_f64)
{
    row_bytes = 0; n_f64 = 0;
    if (n_columns < 1 || n_columns > MAX_COLUMNS || !types || !rows_fit(n_rows, first_row)) return false;
    const int less_row = ROW_DIGITS - digits_of(first_row + (n_rows ? n_rows - 1 : 0));
    const int less_index = ROW_DIGITS - digits_of(n_rows ? n_rows - 1 : 0);
    int bytes = ROW_OVERHEAD - less_row + (with_index ? INDEX_CELL - less_row - less_index : 0);
    for (int c = 0; c < n_columns; ++c) {
        if (types[c] < 0 || types[c] >= tablep::N_TYPES) return false;
        bytes += CELL_OVERHEAD - less_row + tablep::FIELD_WIDTH[types[c]];
        n_f64 += types[c] == tablep::COL_F64;
    }
    row_bytes = bytes;
    return true;
}

// prefix, n_rows longest rows, suffix; false: rows outside the sheet, arithmetic beyond size_t, or more than the 32-bit scans hold
inline bool bound_of(long long n_rows, long long first_row, int row_bytes, size_t prefix_bytes, size_t suffix_bytes, size_t &bound)
{
    bound = 0;
    if (!rows_fit(n_rows, first_row) || row_bytes <= 0) return false;
    size_t text, all;
    if (__builtin_mul_overflow((size_t)n_rows, (size_t)row_bytes, &text) || __builtin_add_overflow(text, prefix_bytes, &all) ||
        __builtin_add_overflow(all, suffix_bytes, &all) || all > MAX_TEXT)
        return false;
    bound = all;
    return true;
}

// the workspace of n_rows >= 0 rows (the suffix waits there for the packing launch, also with no row); false as bound_of
inline bool plan_of(long long n_rows, long long first_row, int n_columns, const int32_t *types, bool with_index, size_t suffix_bytes, Plan &p)
{
    size_t text;
    if (!row_of(n_columns, types, with_index, n_rows, first_row, p.row_bytes, p.n_f64) || !bound_of(n_rows, first_row, p.row_bytes, 0, suffix_bytes, text)) return false;
    const size_t n = (size_t)n_rows;
    p.row_stride = (p.row_bytes + 3) / 4 * 4;
    p.groups = (n + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP;
    p.piece_stride = ((size_t)ROWS_PER_GROUP * (size_t)p.row_bytes + 15) / 16 * 16 + 16;
    return tablep::layout_of(n, p.n_f64, p.groups, p.piece_stride, suffix_bytes + 1, p);
}

}  // namespace xlsxp
