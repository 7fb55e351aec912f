// libysmr_hip -- a table of typed columns as the text DataFrame.to_csv(index=False) writes (helper_file.py:1366-1400:
// save_df_to_csv, the printer of <name>_selected_data.csv and <name>_analysed.csv), printed on the device from columns that
// are there.  rows.hip prints ONE table, the list of ysmr_row under its fixed header; this source takes up to sixteen columns
// of five types and the header as bytes.
//
//   k_table_prepass   a lane per row: how many of its float64 cells are WIDE (finite, non-zero, outside fmt.h's in_range)
//   (prim.h scan)     inclusive sums: the wide cells are numbered in (row, column) order
//   k_table_wide      a small fixed grid that reads their number from device memory (no host synchronisation): wide cell j is
//                     found by a search in the sums, printed by fmt.h's shortest_wide into side slot j (24 bytes) -- the only
//                     kernel here that uses scratch memory, for its 1152-bit integers
//   k_table_rows      a lane per row, 128 rows per workgroup: every value is printed once, straight into the row's place in
//                     LDS (a stride of the widest row the DECLARED types can give), wide cells copied from their slots; a
//                     prefix sum over the rows' lengths (wave shuffles, then the two waves) and the workgroup's text leaves
//                     for HBM compacted, as one piece, in 16-byte stores a lane each
//   (prim.h scan)     inclusive sums of the pieces' lengths
//   k_table_pack      a workgroup per piece: the piece to its place behind the header, 16-byte stores on the destination's
//                     alignment, the source realigned in registers; one more workgroup for a suffix behind the last piece
//                     (the csv has none) and the length
// The text is a function of the input alone: no place comes from an atomic.  The host-only arithmetic is table_csv_plan.h.
// Who owns what: this source owns the csv line (table_csv_row.h) and the loop of k_table_rows over its cells, and it DEFINES
// what table_print.h declares for every printer of typed columns -- check_columns, types_of, the wide-cell kernels behind
// launch_wide_cells, k_table_pack behind launch_pack.  The row kernel's tail and the float64 cell are table_print.h's templates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "common.h"
#include "prim.h"
#include "fmt.h"
#include "table_csv_plan.h"
#include "table_csv_row.h"
#include "table_print.h"

static_assert(tablep::SCAN_TILE == ysmr::prim::SCAN_TILE, "table_csv_plan.h restates prim.h's scan tile");
static_assert(tablep::COL_U32 == YSMR_COL_U32 && tablep::COL_I64 == YSMR_COL_I64 && tablep::COL_I32 == YSMR_COL_I32 &&
              tablep::COL_I8 == YSMR_COL_I8 && tablep::COL_F64 == YSMR_COL_F64, "table_csv_plan.h restates the column types");

namespace {

constexpr int R = tablep::ROWS_PER_GROUP;
constexpr int WIDE_GRID = 256;                     // workgroups of k_table_wide, a wave each

using tablep::Columns;

__global__ __launch_bounds__(256) void k_table_prepass(Columns cols, long long n_rows, uint32_t *__restrict__ wide_count)
{
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n_rows; row += (long long)gridDim.x * 256) {
        uint32_t wide = 0;
#pragma unroll 1
        for (int c = 0; c < cols.n; ++c)
            if (cols.type[c] == YSMR_COL_F64) wide += ysmr_fmt::is_wide_cell(((const double *)cols.data[c])[row]) ? 1u : 0u;
        wide_count[row] = wide;
    }
}

__global__ __launch_bounds__(64) void k_table_wide(Columns cols, long long n_rows, const uint32_t *__restrict__ wide_incl,
                                                  char *__restrict__ slots, uint8_t *__restrict__ slot_len, uint32_t *wide_cells)
{
    const uint32_t total = wide_incl[n_rows - 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) *wide_cells = total;
    for (uint32_t j = blockIdx.x * 64u + threadIdx.x; j < total; j += gridDim.x * 64u) {
        long long lo = 0, hi = n_rows - 1;                       // the first row whose inclusive sum exceeds j holds cell j
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (wide_incl[mid] > j) hi = mid; else lo = mid + 1;
        }
        uint32_t k = j - (lo ? wide_incl[lo - 1] : 0u);          // ... as its k-th wide cell
        double v = 0.0;
        for (int c = 0; c < cols.n; ++c) {
            if (cols.type[c] != YSMR_COL_F64) continue;
            v = ((const double *)cols.data[c])[lo];
            if (!ysmr_fmt::is_wide_cell(v)) continue;
            if (k == 0) break;
            --k;
        }
        char text[tablep::WIDE_SLOT];
        const int len = (int)(ysmr_fmt::put_f64_wide(text, v) - text);
        char *slot = slots + (size_t)j * tablep::WIDE_SLOT;
        for (int b = 0; b < len; ++b) slot[b] = text[b];
        slot_len[j] = (uint8_t)len;
    }
}

extern __shared__ __align__(16) char s_text[];      // R rows of row_stride bytes

__global__ __launch_bounds__(R) void k_table_rows(Columns cols, long long n_rows, int row_stride, const uint32_t *__restrict__ wide_incl,
                                                  const char *__restrict__ slots, const uint8_t *__restrict__ slot_len,
                                                  char *__restrict__ pieces, size_t piece_stride, uint32_t *__restrict__ piece_len)
{
    __shared__ uint32_t s_off[R + 1];               // where row r begins in the piece; s_off[R] is the piece's length
    __shared__ uint32_t s_wave[R / 64];
    __shared__ ysmr_fmt::Digits s_digits[R];        // (a lane's digits, indexed as they come: in LDS this costs no scratch)
    const int lane = threadIdx.x;
    const long long row = (long long)blockIdx.x * R + lane;
    char *const mine = s_text + (size_t)lane * row_stride;
    uint32_t len = 0;
    if (row < n_rows) {
        char *q = mine;
        uint32_t wide_at = (wide_incl && row) ? wide_incl[row - 1] : 0u;
#pragma unroll 1
        for (int c = 0; c < cols.n; ++c) {
            const void *data = cols.data[c];
            const int type = cols.type[c];
            if (type == YSMR_COL_F64)
                q = tablep::put_f64_cell(q, ((const double *)data)[row], slots, slot_len, wide_at, s_digits[lane]);
            else q = tablep::put_int_cell(q, type, data, row);
            *q++ = ',';
        }
        len = (uint32_t)(tablep::end_line(mine, q) - mine);
    }
    tablep::store_piece<R>(len, s_text, row_stride, s_off, s_wave, pieces, piece_stride, piece_len);
}

// (the head: it is in out[0, head) already.)  Workgroups 0 .. n_pieces - 1 move a piece each; workgroup n_pieces writes the
// suffix behind the last piece, and the length
__global__ __launch_bounds__(256) void k_table_pack(const char *__restrict__ pieces, size_t piece_stride, const uint32_t *__restrict__ piece_len,
                                                    const uint32_t *__restrict__ piece_incl, unsigned n_pieces, size_t head,
                                                    const char *__restrict__ suffix, uint32_t suffix_bytes, char *__restrict__ out,
                                                    size_t capacity, unsigned long long *out_length)
{
    if (blockIdx.x >= n_pieces) {
        const size_t at = head + (n_pieces ? piece_incl[n_pieces - 1] : 0u);
        for (uint32_t b = threadIdx.x; b < suffix_bytes; b += 256u)
            if (at + b < capacity) out[at + b] = suffix[b];
        if (threadIdx.x == 0) *out_length = (unsigned long long)at + suffix_bytes;
        return;
    }
    const uint32_t len = piece_len[blockIdx.x];
    const size_t at = head + (size_t)(piece_incl[blockIdx.x] - len);
    const char *src = pieces + (size_t)blockIdx.x * piece_stride;          // 16-byte aligned, 16 bytes of slack behind the text
    const uint32_t to_boundary = (uint32_t)((16u - (at & 15u)) & 15u);
    const uint32_t lead = to_boundary < len ? to_boundary : len;
    const uint32_t body = (len - lead) / 16u, tail_at = lead + body * 16u;
    for (uint32_t b = threadIdx.x; b < lead; b += 256u)
        if (at + b < capacity) out[at + b] = src[b];
    for (uint32_t b = tail_at + threadIdx.x; b < len; b += 256u)
        if (at + b < capacity) out[at + b] = src[b];
    const uint32_t shift = (lead & 3u) * 8u;
    const uint32_t *words = (const uint32_t *)src + (lead >> 2);
    uint4 *dst = (uint4 *)(out + at + lead);
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

int check_bound(long long n_rows, int n_columns, const int32_t *types, size_t header_bytes, size_t capacity, size_t &bound)
{
    int row_bytes = 0, n_f64 = 0;
    tablep::row_of(n_columns, types, row_bytes, n_f64);
    if (n_rows < 0) return ysmr::fail(YSMR_ERR_ARG, "n_rows must not be negative, got %lld", n_rows);
    if (!tablep::bound_of(n_rows, row_bytes, header_bytes, bound))
        return ysmr::fail(YSMR_ERR_CAPACITY, "%lld rows of up to %d bytes behind a header of %zu: more than the 32-bit offsets hold", n_rows,
                          row_bytes, header_bytes);
    if (capacity < bound) return ysmr::fail(YSMR_ERR_CAPACITY, "csv buffer too small: %zu < %zu bytes", capacity, bound);
    return YSMR_OK;
}

}  // namespace

// the types of the columns, or why the call is refused
int tablep::check_columns(int n_columns, const ysmr_table_column *columns, long long n_rows, int32_t *types)
{
    if (n_columns < 1 || n_columns > tablep::MAX_COLUMNS)
        return ysmr::fail(YSMR_ERR_ARG, "n_columns must be in 1..%d, got %d", tablep::MAX_COLUMNS, n_columns);
    if (!columns) return ysmr::fail(YSMR_ERR_ARG, "columns must be set");
    for (int c = 0; c < n_columns; ++c) {
        if (columns[c].type < 0 || columns[c].type >= tablep::N_TYPES)
            return ysmr::fail(YSMR_ERR_ARG, "column %d: unknown type %d", c, (int)columns[c].type);
        if (n_rows > 0 && !columns[c].data) return ysmr::fail(YSMR_ERR_ARG, "column %d: data is NULL", c);
        types[c] = columns[c].type;
    }
    return YSMR_OK;
}

bool tablep::types_of(int n_columns, const ysmr_table_column *columns, int32_t *types)
{
    if (n_columns < 1 || n_columns > tablep::MAX_COLUMNS || !columns) return false;
    for (int c = 0; c < n_columns; ++c) types[c] = columns[c].type;
    return true;
}

void tablep::launch_wide_cells(hipStream_t st, int n_columns, const void *const *data, const int32_t *types, long long n_rows,
                               uint32_t *wide_incl, uint32_t *wide_temp, char *slots, uint8_t *slot_len, uint32_t *wide_cells_dev)
{
    Columns cols{};
    cols.n = n_columns;
    for (int c = 0; c < n_columns; ++c) { cols.data[c] = data[c]; cols.type[c] = types[c]; }
    const unsigned grid = (unsigned)std::min<long long>((n_rows + 255) / 256, 2048);
    hipLaunchKernelGGL(k_table_prepass, dim3(grid), dim3(256), 0, st, cols, n_rows, wide_incl);
    ysmr::prim::inclusive_scan_u32(st, wide_incl, wide_incl, (size_t)n_rows, wide_temp);
    hipLaunchKernelGGL(k_table_wide, dim3(WIDE_GRID), dim3(64), 0, st, cols, n_rows, (const uint32_t *)wide_incl, slots, slot_len, wide_cells_dev);
}

void tablep::launch_pack(hipStream_t st, const char *pieces, size_t piece_stride, const uint32_t *piece_len, const uint32_t *piece_incl,
                         unsigned n_pieces, size_t head, const char *suffix_dev, uint32_t suffix_bytes, char *out, size_t capacity,
                         unsigned long long *length_dev)
{
    hipLaunchKernelGGL(k_table_pack, dim3(n_pieces + 1u), dim3(256), 0, st, pieces, piece_stride, piece_len, piece_incl, n_pieces, head,
                       suffix_dev, suffix_bytes, out, capacity, length_dev);
}

extern "C" {

size_t ysmr_table_csv_bound(long long n_rows, int n_columns, const ysmr_table_column *columns, size_t header_bytes)
{
    int32_t types[tablep::MAX_COLUMNS];
    int row_bytes = 0, n_f64 = 0;
    size_t bound = 0;
    if (!tablep::types_of(n_columns, columns, types) || !tablep::row_of(n_columns, types, row_bytes, n_f64) ||
        !tablep::bound_of(n_rows, row_bytes, header_bytes, bound))
        return 0;
    return bound;
}

// (n_rows = 0 needs no workspace: 256, so that 0 always means refused)
size_t ysmr_table_format_workspace_bytes(long long n_rows, int n_columns, const ysmr_table_column *columns)
{
    int32_t types[tablep::MAX_COLUMNS];
    int row_bytes = 0, n_f64 = 0;
    if (!tablep::types_of(n_columns, columns, types) || !tablep::row_of(n_columns, types, row_bytes, n_f64)) return 0;
    if (n_rows == 0) return 256;
    tablep::Plan p{};
    return tablep::plan_of(n_rows, n_columns, types, p) ? p.total : 0;
}

void ysmr_table_format_geometry(int *rows_per_group, int *staged_bytes)
{
    if (rows_per_group) *rows_per_group = tablep::ROWS_PER_GROUP;
    if (staged_bytes) *staged_bytes = tablep::STAGED_BYTES;
}

int ysmr_table_format_device(void *stream, long long n_rows, int n_columns, const ysmr_table_column *columns, const char *header_host,
                             size_t header_bytes, void *workspace_dev, size_t workspace_bytes, char *csv_dev, size_t csv_capacity,
                             unsigned long long *csv_length_dev, uint32_t *wide_cells_dev)
{
    int32_t types[tablep::MAX_COLUMNS];
    if (const int rc = tablep::check_columns(n_columns, columns, n_rows, types)) return rc;
    if (!csv_dev || !csv_length_dev || !wide_cells_dev || (header_bytes && !header_host))
        return ysmr::fail(YSMR_ERR_ARG, "header_host, csv_dev, csv_length_dev and wide_cells_dev must be set");
    size_t bound = 0;
    if (const int rc = check_bound(n_rows, n_columns, types, header_bytes, csv_capacity, bound)) return rc;
    tablep::Plan p{};
    if (n_rows) {
        if (!tablep::plan_of(n_rows, n_columns, types, p))
            return ysmr::fail(YSMR_ERR_CAPACITY, "the workspace of %lld rows does not fit a size_t", n_rows);
        if (!workspace_dev) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be set");
        if (workspace_bytes < p.total)
            return ysmr::fail(YSMR_ERR_CAPACITY, "table workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    }
    hipStream_t st = (hipStream_t)stream;
    if (header_bytes) YSMR_HIP_CHECK(hipMemcpyAsync(csv_dev, header_host, header_bytes, hipMemcpyHostToDevice, st));
    char *w = (char *)workspace_dev;
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
        hipLaunchKernelGGL(k_table_rows, dim3((unsigned)p.groups), dim3(R), (size_t)R * p.row_stride, st, cols, n_rows, p.row_stride,
                           (const uint32_t *)wide_incl, (const char *)slots, (const uint8_t *)slot_len, w + p.pieces, p.piece_stride, piece_len);
        ysmr::prim::inclusive_scan_u32(st, piece_len, piece_incl, p.groups, (uint32_t *)(w + p.piece_temp));
    }
    // (no row: p is empty, no piece, and the packing launch writes the header's length alone)
    tablep::launch_pack(st, w + p.pieces, p.piece_stride, piece_len, piece_incl, (unsigned)p.groups, header_bytes, nullptr, 0, csv_dev, csv_capacity,
                        csv_length_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

// the same arithmetic (fmt.h) on the HOST, a row at a time, on columns in host memory
int ysmr_table_format_devicelike(long long n_rows, int n_columns, const ysmr_table_column *columns, const char *header, size_t header_bytes,
                                 char *out, size_t out_capacity, size_t *out_length, long long *wide_cells)
{
    int32_t types[tablep::MAX_COLUMNS];
    if (const int rc = tablep::check_columns(n_columns, columns, n_rows, types)) return rc;
    if (!out || !out_length || !wide_cells || (header_bytes && !header))
        return ysmr::fail(YSMR_ERR_ARG, "header, out, out_length and wide_cells must be set");
    size_t bound = 0;
    if (const int rc = check_bound(n_rows, n_columns, types, header_bytes, out_capacity, bound)) return rc;
    char *p = out;
    if (header_bytes) { std::memcpy(p, header, header_bytes); p += header_bytes; }
    long long wide = 0;
    const void *data[tablep::MAX_COLUMNS];
    for (int c = 0; c < n_columns; ++c) data[c] = columns[c].data;
    for (long long row = 0; row < n_rows; ++row) p = tablep::put_row(p, n_columns, types, data, row, &wide);
    *out_length = (size_t)(p - out);
    *wide_cells = wide;
    return YSMR_OK;
}

// HOST: the text of n float64 fields, 24-byte slots (zero filled behind the text) and their lengths.  printer 0: fmt.h's
// shortest() where it applies (255 as the length of a value it declines), 1: shortest_wide() for every finite non-zero value,
// 2: the writer's choice between the two
int ysmr_fmt_f64_text(const double *values, long long n, int printer, char *slots, uint8_t *lengths)
{
    if (n < 0 || (n && (!values || !slots || !lengths)) || printer < 0 || printer > 2)
        return ysmr::fail(YSMR_ERR_ARG, "values, slots and lengths must be set and printer be 0, 1 or 2");
    auto work = [=](long long lo, long long hi) {
        for (long long i = lo; i < hi; ++i) {
            char *slot = slots + (size_t)i * tablep::WIDE_SLOT;
            std::memset(slot, 0, tablep::WIDE_SLOT);
            const double v = values[i];
            const uint64_t a = ysmr_fmt::bits_of(v) & 0x7FFFFFFFFFFFFFFFull;
            const bool plain = a == 0 || a >= 0x7FF0000000000000ull;          // zero, infinities, NaN: no digits to work out
            char *end;
            if (printer == 2 || plain) end = ysmr_fmt::put_f64_field(slot, v);
            else if (printer == 1) end = ysmr_fmt::put_f64_wide(slot, v);
            else if (ysmr_fmt::is_wide_cell(v)) { lengths[i] = 255; continue; }
            else { ysmr_fmt::Digits g; end = ysmr_fmt::put_f64_steady(slot, v, g); }
            lengths[i] = (uint8_t)(end - slot);
        }
    };
    const int nt = n < 4096 ? 1 : (int)std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
    if (nt == 1) { work(0, n); return YSMR_OK; }
    std::vector<std::thread> pool;
    const long long per = (n + nt - 1) / nt;
    int started = 0;
    try {
        for (; started < nt - 1; ++started) pool.emplace_back(work, std::min<long long>(started * per, n), std::min<long long>((started + 1) * per, n));
    } catch (const std::system_error &) {
    }
    work(std::min<long long>(started * per, n), n);
    for (auto &th : pool) th.join();
    return YSMR_OK;
}

}  // extern "C"
