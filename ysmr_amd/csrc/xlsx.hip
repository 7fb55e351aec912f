// libysmr_hip -- a table of typed columns as the rows of a worksheet of an .xlsx workbook (helper_file.py:92-137 upstream:
// collate_results_csv_to_xlsx, DataFrame.to_excel of every `*statistics.csv`), printed on the device from columns that are
// there.  The structure is table_csv.hip's, the row is xlsx_row.h's instead of a csv line:
//   (table_wide.h)    the wide float64 cells into their side slots: table_csv.hip's pre-pass, scan and wide printer as they are
//   k_xlsx_rows       a lane per row, 64 rows (a wave) per workgroup: every value is printed once, straight into the row's place
//                     in LDS (a stride of the longest row the DECLARED types can give), wide cells copied from their slots; a
//                     prefix sum over the rows' lengths (wave shuffles) and the workgroup's text leaves for HBM compacted, as
//                     one piece, in 16-byte stores a lane each
//   (prim.h scan)     inclusive sums of the pieces' lengths
//   k_xlsx_pack       a workgroup per piece: the piece to its place behind the prefix, 16-byte stores on the destination's
//                     alignment, the source realigned in registers; the suffix behind the last piece, and the length
// The text is a function of the input alone: no place comes from an atomic.  The host-only arithmetic is xlsx_plan.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.h"
#include "prim.h"
#include "fmt.h"
#include "table_wide.h"
#include "xlsx_plan.h"
#include "xlsx_row.h"

namespace {

constexpr int R = xlsxp::ROWS_PER_GROUP;
static_assert(R == 64, "k_xlsx_rows is one wave: its prefix sum is wave_inclusive_sum alone");

struct Columns {
    const void *data[xlsxp::MAX_COLUMNS];
    int32_t type[xlsxp::MAX_COLUMNS];
    int32_t n;
};

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
                if (ysmr_fmt::is_wide_cell(v)) {
                    const char *slot = slots + (size_t)wide_at * tablep::WIDE_SLOT;
                    const int l = slot_len[wide_at];
                    for (int b = 0; b < l; ++b) q[b] = slot[b];
                    q += l;
                    ++wide_at;
                } else q = ysmr_fmt::put_f64_steady(q, v, s_digits[lane]);
            } else {
                q = xlsxp::cell_open(q, column, sheet_row, false);
                q = tablep::put_int_cell(q, type, data, row);
            }
            q = xlsxp::cell_close(q);
        }
        len = (uint32_t)(xlsxp::row_close(q) - mine);
    }
    // where every row goes in the piece
    const uint32_t incl = ysmr::prim::wave_inclusive_sum(len);
    if (lane == 0) s_off[0] = 0u;
    s_off[lane + 1] = incl;
    __syncthreads();
    const uint32_t total = s_off[R];
    if (lane == 0) piece_len[blockIdx.x] = total;
    // the piece leaves compacted: lane after lane sixteen consecutive bytes of it, gathered from the rows they lie in
    uint4 *const out = (uint4 *)(pieces + (size_t)blockIdx.x * piece_stride);
    for (uint32_t chunk = (uint32_t)lane; chunk * 16u < total; chunk += (uint32_t)R) {
        const uint32_t first = chunk * 16u;
        int r = 0;
#pragma unroll
        for (int step = R / 2; step; step >>= 1)                 // the last row that begins at or before `first`
            if (s_off[r + step] <= first) r += step;
        uint32_t pos = first - s_off[r], row_len = s_off[r + 1] - s_off[r];
        const char *src = s_text + (size_t)r * row_stride;
        uint32_t word[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (first + 4u * k + b < total) {
                    w |= (uint32_t)(uint8_t)src[pos] << (8 * b);
                    if (++pos == row_len && r + 1 < R) { ++r; src += row_stride; pos = 0; row_len = s_off[r + 1] - s_off[r]; }
                }
            }
            word[k] = w;
        }
        out[chunk] = make_uint4(word[0], word[1], word[2], word[3]);
    }
}

// (prefix: it is in xml[0, head) already.)  Workgroups 0 .. n_pieces - 1 move a piece each, workgroup n_pieces the suffix
__global__ __launch_bounds__(256) void k_xlsx_pack(const char *__restrict__ pieces, size_t piece_stride, const uint32_t *__restrict__ piece_len,
                                                   const uint32_t *__restrict__ piece_incl, unsigned n_pieces, size_t head,
                                                   const char *__restrict__ suffix, uint32_t suffix_bytes, char *__restrict__ xml,
                                                   size_t capacity, unsigned long long *xml_length)
{
    if (blockIdx.x >= n_pieces) {
        const size_t at = head + (n_pieces ? piece_incl[n_pieces - 1] : 0u);
        for (uint32_t b = threadIdx.x; b < suffix_bytes; b += 256u)
            if (at + b < capacity) xml[at + b] = suffix[b];
        if (threadIdx.x == 0) *xml_length = (unsigned long long)at + suffix_bytes;
        return;
    }
    const uint32_t len = piece_len[blockIdx.x];
    const size_t at = head + (size_t)(piece_incl[blockIdx.x] - len);
    const char *src = pieces + (size_t)blockIdx.x * piece_stride;          // 16-byte aligned, 16 bytes of slack behind the text
    const uint32_t to_boundary = (uint32_t)((16u - (at & 15u)) & 15u);
    const uint32_t lead = to_boundary < len ? to_boundary : len;
    const uint32_t body = (len - lead) / 16u, tail_at = lead + body * 16u;
    for (uint32_t b = threadIdx.x; b < lead; b += 256u)
        if (at + b < capacity) xml[at + b] = src[b];
    for (uint32_t b = tail_at + threadIdx.x; b < len; b += 256u)
        if (at + b < capacity) xml[at + b] = src[b];
    const uint32_t shift = (lead & 3u) * 8u;
    const uint32_t *words = (const uint32_t *)src + (lead >> 2);
    uint4 *dst = (uint4 *)(xml + at + lead);
    for (uint32_t i = threadIdx.x; i < body; i += 256u) {
        uint32_t w[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) w[k] = words[4u * i + k];
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (uint32_t)((((uint64_t)w[k + 1] << 32) | w[k]) >> shift);
        if (at + lead + 16ull * i + 16ull <= capacity) dst[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// the types of the columns, or why the call is refused
int check_columns(int n_columns, const ysmr_table_column *columns, long long n_rows, int32_t *types)
{
    if (n_columns < 1 || n_columns > xlsxp::MAX_COLUMNS)
        return ysmr::fail(YSMR_ERR_ARG, "n_columns must be in 1..%d, got %d", xlsxp::MAX_COLUMNS, n_columns);
    if (!columns) return ysmr::fail(YSMR_ERR_ARG, "columns must be set");
    for (int c = 0; c < n_columns; ++c) {
        if (columns[c].type < 0 || columns[c].type >= tablep::N_TYPES)
            return ysmr::fail(YSMR_ERR_ARG, "column %d: unknown type %d", c, (int)columns[c].type);
        if (n_rows > 0 && !columns[c].data) return ysmr::fail(YSMR_ERR_ARG, "column %d: data is NULL", c);
        types[c] = columns[c].type;
    }
    return YSMR_OK;
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

bool types_of(int n_columns, const ysmr_table_column *columns, int32_t *types)
{
    if (n_columns < 1 || n_columns > xlsxp::MAX_COLUMNS || !columns) return false;
    for (int c = 0; c < n_columns; ++c) types[c] = columns[c].type;
    return true;
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
    hipLaunchKernelGGL(k_xlsx_pack, dim3((unsigned)p.groups + 1u), dim3(256), 0, st, (const char *)(w + p.pieces), p.piece_stride,
                       (const uint32_t *)piece_len, (const uint32_t *)piece_incl, (unsigned)p.groups, prefix_bytes, (const char *)(w + p.suffix),
                       (uint32_t)suffix_bytes, xml_dev, xml_capacity, xml_length_dev);
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
