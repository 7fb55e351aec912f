// libysmr_hip -- a table of typed columns as the rows of a worksheet of an .xlsx workbook (helper_file.py:92-137 upstream:
// collate_results_csv_to_xlsx, DataFrame.to_excel of every `*statistics.csv`), printed on the device from columns that are
// there.
//   (launch_wide_cells) the wide float64 cells into their side slots: table_csv.hip's pre-pass, scan and wide printer
//   k_xlsx_rows       a lane per row, 64 rows (a wave) per workgroup: every value is printed once, straight into the row's place
//                     in LDS (a stride of the longest row the DECLARED types can give), wide cells copied from their slots;
//                     then table_print.h's tail: the prefix sum over the rows' lengths and the compacted piece
//   (prim.h scan)     inclusive sums of the pieces' lengths
//   (launch_pack)     table_csv.hip's k_table_pack: the pieces behind the prefix, the suffix behind the last piece, the length
// Who owns what: this source owns the worksheet row (xlsx_row.h), the loop of k_xlsx_rows over its cells, and the sheet's
// bound and geometry (xlsx_plan.h).  Staging, compaction, the wide cells, the packing kernel, the column checks and the
// workspace layout are table_print.h's and table_csv_plan.h's, shared with the csv printer.
// The text is a function of the input alone: no place comes from an atomic.
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.h"
#include "prim.h"
#include "fmt.h"
#include "table_print.h"
#include "xlsx_plan.h"
#include "xlsx_row.h"

namespace {

constexpr int R = xlsxp::ROWS_PER_GROUP;
static_assert(R == 64, "k_xlsx_rows is one wave: the shared tail needs no s_wave and one barrier");
using tablep::Columns;
using tablep::check_columns;
using tablep::types_of;

extern __shared__ __align__(16) char s_text[];      // R rows of row_stride bytes

__global__ __launch_bounds__(R) void k_xlsx_rows(Columns cols, long long n_rows, uint32_t first_row, int with_index, int row_stride,
                                                 const uint32_t *__restrict__ wide_incl, const char *__restrict__ slots,
                                                 const uint8_t *__restrict__ slot_len, char *__restrict__ pieces, size_t piece_stride,
                                                 uint32_t *__restrict__ piece_len)
{
    __shared__ uint32_t s_off[R + 1];               // where row r begins in the piece; s_off[R] is the piece's length
    __shared__ ysmr_fmt::Digits s_digits[R];        // (a lane's digits, indexed as they come: in LDS this costs no scratch)
    const int lane = threadIdx.x;
    const long long row = (long long)blockIdx.x * R + lane;
    char *const mine = s_text + (size_t)lane * row_stride;
    uint32_t len = 0;
    if (row < n_rows) {
        const uint32_t sheet_row = first_row + (uint32_t)row;
        char *q = xlsxp::row_open(mine, sheet_row);
        if (with_index) q = xlsxp::index_cell(q, sheet_row, (uint32_t)row);
        uint32_t wide_at = (wide_incl && row) ? wide_incl[row - 1] : 0u;
#pragma unroll 1
        for (int c = 0; c < cols.n; ++c) {
            const void *data = cols.data[c];
            const int type = cols.type[c];
            const int column = c + (with_index ? 1 : 0);
            if (type == YSMR_COL_F64) {
                const double v = ((const double *)data)[row];
                if (xlsxp::is_nan(v)) continue;
                q = xlsxp::cell_open(q, column, sheet_row, xlsxp::is_inf(v));
                q = tablep::put_f64_cell(q, v, slots, slot_len, wide_at, s_digits[lane]);
            } else {
                q = xlsxp::cell_open(q, column, sheet_row, false);
                q = tablep::put_int_cell(q, type, data, row);
            }
            q = xlsxp::cell_close(q);
        }
        len = (uint32_t)(xlsxp::row_close(q) - mine);
    }
    tablep::store_piece<R>(len, s_text, row_stride, s_off, nullptr, pieces, piece_stride, piece_len);
}

int check_bound(long long n_rows, long long first_row, int n_columns, const int32_t *types, bool with_index, size_t prefix_bytes,
                size_t suffix_bytes, size_t capacity, size_t &bound)
{
    int row_bytes = 0, n_f64 = 0;
    if (!xlsxp::row_of(n_columns, types, with_index, n_rows, first_row, row_bytes, n_f64))
        return ysmr::fail(YSMR_ERR_ARG, "%lld rows from sheet row %lld do not lie in 1..%lld", n_rows, first_row, xlsxp::MAX_SHEET_ROW);
    if (!xlsxp::bound_of(n_rows, first_row, row_bytes, prefix_bytes, suffix_bytes, bound))
        return ysmr::fail(YSMR_ERR_CAPACITY, "%lld rows of up to %d bytes between %zu and %zu: more than the 32-bit offsets hold", n_rows,
                          row_bytes, prefix_bytes, suffix_bytes);
    if (capacity < bound) return ysmr::fail(YSMR_ERR_CAPACITY, "sheet buffer too small: %zu < %zu bytes", capacity, bound);
    return YSMR_OK;
}

}  // namespace

extern "C" {

size_t ysmr_xlsx_sheet_bound(long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row, int with_index,
                             size_t prefix_bytes, size_t suffix_bytes)
{
    int32_t types[xlsxp::MAX_COLUMNS];
    int row_bytes = 0, n_f64 = 0;
    size_t bound = 0;
    if (!types_of(n_columns, columns, types) || !xlsxp::row_of(n_columns, types, with_index != 0, n_rows, first_row, row_bytes, n_f64) ||
        !xlsxp::bound_of(n_rows, first_row, row_bytes, prefix_bytes, suffix_bytes, bound))
        return 0;
    return bound;
}

// (never 0 for what is served: the suffix waits in the workspace, also with no row)
size_t ysmr_xlsx_sheet_workspace_bytes(long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row, int with_index,
                                       size_t suffix_bytes)
{
    int32_t types[xlsxp::MAX_COLUMNS];
    xlsxp::Plan p{};
    if (!types_of(n_columns, columns, types) || !xlsxp::plan_of(n_rows, first_row, n_columns, types, with_index != 0, suffix_bytes, p)) return 0;
    return p.total;
}

void ysmr_xlsx_sheet_geometry(int *rows_per_group, int *staged_bytes, int *max_row_bytes)
{
    if (rows_per_group) *rows_per_group = xlsxp::ROWS_PER_GROUP;
    if (staged_bytes) *staged_bytes = xlsxp::STAGED_BYTES;
    if (max_row_bytes) *max_row_bytes = xlsxp::MAX_ROW_BYTES;
}

int ysmr_xlsx_sheet_device(void *stream, long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row,
                           int with_index, const char *prefix_host, size_t prefix_bytes, const char *suffix_host, size_t suffix_bytes,
                           void *workspace_dev, size_t workspace_bytes, char *xml_dev, size_t xml_capacity,
                           unsigned long long *xml_length_dev, uint32_t *wide_cells_dev)
{
    int32_t types[xlsxp::MAX_COLUMNS];
    if (const int rc = check_columns(n_columns, columns, n_rows, types)) return rc;
    if (!xml_dev || !xml_length_dev || !wide_cells_dev || (prefix_bytes && !prefix_host) || (suffix_bytes && !suffix_host))
        return ysmr::fail(YSMR_ERR_ARG, "prefix_host, suffix_host, xml_dev, xml_length_dev and wide_cells_dev must be set");
    size_t bound = 0;
    if (const int rc = check_bound(n_rows, first_row, n_columns, types, with_index != 0, prefix_bytes, suffix_bytes, xml_capacity, bound)) return rc;
    xlsxp::Plan p{};
    if (!xlsxp::plan_of(n_rows, first_row, n_columns, types, with_index != 0, suffix_bytes, p))
        return ysmr::fail(YSMR_ERR_CAPACITY, "the workspace of %lld rows does not fit a size_t", n_rows);
    if (!workspace_dev || ((uintptr_t)workspace_dev & 15u)) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be set and 16-byte aligned");
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "sheet workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)workspace_dev;
    if (prefix_bytes) YSMR_HIP_CHECK(hipMemcpyAsync(xml_dev, prefix_host, prefix_bytes, hipMemcpyHostToDevice, st));
    if (suffix_bytes) YSMR_HIP_CHECK(hipMemcpyAsync(w + p.suffix, suffix_host, suffix_bytes, hipMemcpyHostToDevice, st));
    const bool wide = p.n_f64 && n_rows;
    if (!wide) YSMR_HIP_CHECK(hipMemsetAsync(wide_cells_dev, 0, sizeof(uint32_t), st));
    uint32_t *piece_len = (uint32_t *)(w + p.piece_len), *piece_incl = (uint32_t *)(w + p.piece_incl);
    if (n_rows) {
        Columns cols{};
        cols.n = n_columns;
        for (int c = 0; c < n_columns; ++c) { cols.data[c] = columns[c].data; cols.type[c] = types[c]; }
        uint32_t *wide_incl = wide ? (uint32_t *)(w + p.wide_incl) : nullptr;
        char *slots = w + p.wide_slots;
        uint8_t *slot_len = (uint8_t *)(w + p.wide_len);
        if (wide) tablep::launch_wide_cells(st, n_columns, cols.data, cols.type, n_rows, wide_incl, (uint32_t *)(w + p.wide_temp), slots, slot_len,
                                            wide_cells_dev);
        hipLaunchKernelGGL(k_xlsx_rows, dim3((unsigned)p.groups), dim3(R), (size_t)R * p.row_stride, st, cols, n_rows, (uint32_t)first_row,
                           with_index ? 1 : 0, p.row_stride, (const uint32_t *)wide_incl, (const char *)slots, (const uint8_t *)slot_len,
                           w + p.pieces, p.piece_stride, piece_len);
        ysmr::prim::inclusive_scan_u32(st, piece_len, piece_incl, p.groups, (uint32_t *)(w + p.piece_temp));
    }
    tablep::launch_pack(st, w + p.pieces, p.piece_stride, piece_len, piece_incl, (unsigned)p.groups, prefix_bytes, w + p.suffix, (uint32_t)suffix_bytes,
                        xml_dev, xml_capacity, xml_length_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

// the same text (xlsx_row.h, fmt.h) on the HOST, a row at a time, on columns in host memory
int ysmr_xlsx_sheet_devicelike(long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row, int with_index,
                               const char *prefix, size_t prefix_bytes, const char *suffix, size_t suffix_bytes, char *out,
                               size_t out_capacity, size_t *out_length, long long *wide_cells)
{
    int32_t types[xlsxp::MAX_COLUMNS];
    if (const int rc = check_columns(n_columns, columns, n_rows, types)) return rc;
    if (!out || !out_length || !wide_cells || (prefix_bytes && !prefix) || (suffix_bytes && !suffix))
        return ysmr::fail(YSMR_ERR_ARG, "prefix, suffix, out, out_length and wide_cells must be set");
    size_t bound = 0;
    if (const int rc = check_bound(n_rows, first_row, n_columns, types, with_index != 0, prefix_bytes, suffix_bytes, out_capacity, bound)) return rc;
    char *p = out;
    if (prefix_bytes) { std::memcpy(p, prefix, prefix_bytes); p += prefix_bytes; }
    long long wide = 0;
    const void *data[xlsxp::MAX_COLUMNS];
    for (int c = 0; c < n_columns; ++c) data[c] = columns[c].data;
    for (long long row = 0; row < n_rows; ++row) p = xlsxp::put_row(p, n_columns, types, data, row, first_row, with_index != 0, &wide);
    if (suffix_bytes) { std::memcpy(p, suffix, suffix_bytes); p += suffix_bytes; }
    *out_length = (size_t)(p - out);
    *wide_cells = wide;
    return YSMR_OK;
}

}  // extern "C"
