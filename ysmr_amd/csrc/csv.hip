// libysmr_hip -- a track table read back from its csv ON THE DEVICE: what helper_file.get_data (pandas.read_csv with upstream's
// dtype and usecols, helper_file.py:860-905, then the "rough check" and sort_list, :1538-1574) gives for a `*_list.csv` or a
// `*_selected_data.csv`, bit for bit, for the files csv_parse.h serves.  The inverse of ysmr_rows_format_device (rows.hip).
//   ysmr_csv_index   one pass over the text with 16-byte loads: a bit per byte (it is a '\n') kept as 16-bit words, the newlines
//                    of every chunk counted by popcount, '"' / '\r' / NUL / bytes >= 0x80 flagged; a prefix sum over the chunks'
//                    counts; a second pass over the BIT MAP ranks every newline and writes the byte offset of every line start
//   ysmr_csv_parse   a line per lane; a workgroup's lines are one contiguous span, staged into LDS with 16-byte loads and
//                    parsed from there.  What lies beyond the staged span (a long line, through skipped columns) is PARSED
//                    FROM GLOBAL MEMORY, byte by byte: it comes out right, only slower
//   ysmr_csv_parse_typed  the same behind the same index, for 1 .. 16 columns of the table writer's five types (uint32, int64,
//                    int32, int8, float64 with an empty field as NaN on request): what annotate_video reads of an `*_analysed.csv`
//   ysmr_csv_column_kinds  the same behind the same index: per column, whether every field is an int64 field, whether every
//                    field is a float64 field or empty, whether one is empty -- what the collated workbook's reader needs to
//                    know before it names the types of ysmr_csv_parse_typed, as pandas.read_csv infers them
//   ysmr_csv_order   stable radix sort of (TRACK_ID << 32 | POSITION_T) with the row number as payload (prim.h), then a gather
//                    of the seven columns
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "common.h"
#include "prim.h"
#include "csv_parse.h"
#include "csv_plan.h"

static_assert(csvp::SCAN_TILE == ysmr::prim::SCAN_TILE && csvp::RADIX_TILE == ysmr::prim::RADIX_TILE, "csv_plan.h restates prim.h");
static_assert(csvp::STAGED_SPAN % 16 == 0 && csvp::ROWS_PER_GROUP == 256, "geometry of the parse");

namespace {

using csvp::INDEX_CHUNK;
using csvp::INDEX_ROUNDS;
using csvp::STAGED_SPAN;

// bytes of w that equal c (some byte does: non-zero; exact as a whole, which is all a flag needs)
__device__ __forceinline__ uint32_t has_byte(uint32_t w, uint32_t c)
{
    const uint32_t x = w ^ (c * 0x01010101u);
    return (x - 0x01010101u) & ~x & 0x80808080u;
}

__device__ __forceinline__ uint32_t newline_bits(uint32_t w)
{
    return (uint32_t)((w & 0xFFu) == '\n') | (uint32_t)(((w >> 8) & 0xFFu) == '\n') << 1 |
           (uint32_t)(((w >> 16) & 0xFFu) == '\n') << 2 | (uint32_t)((w >> 24) == '\n') << 3;
}

__device__ __forceinline__ uint32_t flags_of(uint32_t w)
{
    return (has_byte(w, '"') ? ysmr_csv::FLAG_QUOTE : 0u) | (has_byte(w, '\r') ? ysmr_csv::FLAG_CR : 0u) |
           ((w & 0x80808080u) || has_byte(w, 0u) ? ysmr_csv::FLAG_NOT_PLAIN : 0u);
}

// A chunk of the text per workgroup: the newline bit map, the chunk's newline count, the file's flags.
// text_dev is 16-byte aligned; bytes behind n_bytes are never read
__global__ __launch_bounds__(256) void k_csv_index(const unsigned char *__restrict__ text, uint32_t n_bytes, uint16_t *__restrict__ bitmap,
                                                   uint32_t *__restrict__ counts, uint32_t *flags_out)
{
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    uint32_t count = 0u, flags = 0u;
#pragma unroll
    for (int r = 0; r < INDEX_ROUNDS; ++r) {
        const size_t word = (size_t)blockIdx.x * (INDEX_CHUNK / 16) + (size_t)r * 256 + threadIdx.x;
        const size_t pos = word * 16;
        uint32_t mask = 0u;
        if (pos + 16 <= (size_t)n_bytes) {
            const uint4 q = *(const uint4 *)(text + pos);
            mask = newline_bits(q.x) | newline_bits(q.y) << 4 | newline_bits(q.z) << 8 | newline_bits(q.w) << 12;
            flags |= flags_of(q.x) | flags_of(q.y) | flags_of(q.z) | flags_of(q.w);
        } else if (pos < (size_t)n_bytes) {
            const int left = (int)((size_t)n_bytes - pos);
            for (int k = 0; k < left; ++k) {
                const uint32_t c = text[pos + k];
                mask |= (uint32_t)(c == '\n') << k;
                // (0x01 fills the word's other bytes: neither a flagged byte nor a zero)
                flags |= flags_of(c | 0x01010100u);
            }
        }
        bitmap[word] = (uint16_t)mask;
        count += (uint32_t)__popc(mask);
    }
    // a wave's counts by shuffles, the four waves' through LDS; the flags only where a wave has any
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) count += (uint32_t)__shfl_down((int)count, d, 64);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(&s_count, count);
    if (__ballot(flags != 0u)) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) flags |= (uint32_t)__shfl_down((int)flags, d, 64);
        if ((threadIdx.x & 63) == 0 && flags) atomicOr(flags_out, flags);
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_count;
}

// counts_incl: inclusive prefix sum of the chunks' newline counts.  starts[0] = 0; starts[k] = the byte behind the k-th '\n';
// behind a last line without '\n' the end mark n_bytes + 1, so that line L is [starts[L], starts[L + 1] - 1) for every line.
// meta: [0] newlines of the file, [1] its lines (a last line without '\n' counts).
__global__ __launch_bounds__(256) void k_csv_starts(const unsigned char *__restrict__ text, uint32_t n_bytes, const uint16_t *__restrict__ bitmap,
                                                    const uint32_t *__restrict__ counts_incl, uint32_t n_chunks, uint32_t *__restrict__ starts,
                                                    uint32_t capacity, uint32_t *meta, uint32_t *n_lines_out, uint32_t *flags_out)
{
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t run = blockIdx.x ? counts_incl[blockIdx.x - 1] : 0u;     // newlines before this round of this chunk
    for (int r = 0; r < INDEX_ROUNDS; ++r) {
        const size_t word = (size_t)blockIdx.x * (INDEX_CHUNK / 16) + (size_t)r * 256 + threadIdx.x;
        uint32_t mask = bitmap[word];
        const uint32_t mine = (uint32_t)__popc(mask);
        const uint32_t incl = ysmr::prim::wave_inclusive_sum(mine);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t rank = run + incl - mine;
        for (int w = 0; w < wave; ++w) rank += s_wave[w];
        run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
        while (mask) {
            const int bit = __ffs((int)mask) - 1;
            mask &= mask - 1u;
            ++rank;                                                    // the line this newline ends is rank - 1
            if (rank < capacity) starts[rank] = (uint32_t)(word * 16) + (uint32_t)bit + 1u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t newlines = counts_incl[n_chunks - 1];
        const bool open_end = text[n_bytes - 1] != '\n';
        const uint32_t lines = newlines + (open_end ? 1u : 0u);
        starts[0] = 0u;
        if (open_end && newlines + 1u < capacity) starts[newlines + 1u] = n_bytes + 1u;
        meta[0] = newlines;
        meta[1] = lines;
        *n_lines_out = lines;
        if ((unsigned long long)lines + 1ull > capacity) atomicOr(flags_out, ysmr_csv::FLAG_TOO_MANY_LINES);
    }
}

struct Columns { uint32_t *id, *t; double *v[5]; };
struct ConstColumns { const uint32_t *id, *t; const double *v[5]; };

// the text of a workgroup's lines: from LDS where it is staged, from global memory beyond
struct StagedText {
    const unsigned char *lds, *text;
    uint32_t a0;
    __device__ __forceinline__ int operator()(long long i) const
    {
        const uint32_t off = (uint32_t)i - a0;
        return off < (uint32_t)STAGED_SPAN ? lds[off] : text[i];
    }
};

__global__ __launch_bounds__(256) void k_csv_parse(const unsigned char *__restrict__ text, uint32_t n_bytes, const uint32_t *__restrict__ starts,
                                                   const uint32_t *__restrict__ meta, int n_columns, ysmr_csv::Wanted wanted,
                                                   uint32_t n_rows, Columns cols, uint32_t *unserved)
{
    __shared__ uint4 s_text[STAGED_SPAN / 16];
    const uint32_t lines = meta[1];
    const uint32_t r0 = blockIdx.x * 256u;
    const uint32_t here = min(256u, n_rows - r0);
    // (row r is line r + 1: the header is line 0.  Rows the index did not find are not read at all.)
    const uint32_t known = r0 + 1u < lines ? min(here, lines - 1u - r0) : 0u;
    uint32_t a0 = 0u;
    if (known) {
        const uint32_t span0 = starts[r0 + 1u], span1 = min(starts[r0 + known + 1u] - 1u, n_bytes);
        a0 = span0 & ~15u;
        const uint32_t stop = min(span1, a0 + (uint32_t)STAGED_SPAN);
        for (uint32_t i = threadIdx.x; a0 + 16u * i < stop && i < (uint32_t)(STAGED_SPAN / 16); i += 256u) {
            const uint32_t pos = a0 + 16u * i;
            if (pos + 16u <= n_bytes) s_text[i] = *(const uint4 *)(text + pos);
            else
                for (uint32_t k = 0; pos + k < n_bytes; ++k) ((unsigned char *)s_text)[16u * i + k] = text[pos + k];
        }
    }
    __syncthreads();
    bool ok = false;
    const uint32_t row = r0 + threadIdx.x;
    if (threadIdx.x < here) {
        ysmr_csv::Row out;
        if (threadIdx.x < known) {
            const uint32_t begin = starts[row + 1u], next = starts[row + 2u];
            if (next > begin && next - 1u <= n_bytes) {
                const StagedText at{(const unsigned char *)s_text, text, a0};
                ok = ysmr_csv::parse_line(at, (long long)begin, (long long)(next - 1u), n_columns, wanted, out);
            }
        }
        if (ok) {
            cols.id[row] = out.id;
            cols.t[row] = out.t;
#pragma unroll
            for (int k = 0; k < 5; ++k) cols.v[k][row] = out.v[k];
        }
    }
    const unsigned long long bad = __ballot(threadIdx.x < here && !ok);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(unserved, (uint32_t)__popcll(bad));
}

struct TypedColumns { void *data[ysmr_csv::MAX_FIELDS]; };

// k_csv_parse for 1 .. 16 typed columns (csv_parse.h: parse_line_typed): the same grid, staging and line-per-lane layout.
// A served row's fields go out in the order of the plan, each a coalesced store of its own width
__global__ __launch_bounds__(256) void k_csv_parse_typed(const unsigned char *__restrict__ text, uint32_t n_bytes,
                                                         const uint32_t *__restrict__ starts, const uint32_t *__restrict__ meta,
                                                         int n_columns, ysmr_csv::TypedPlan plan, uint32_t n_rows, TypedColumns cols,
                                                         uint32_t *unserved)
{
    __shared__ uint4 s_text[STAGED_SPAN / 16];
    const uint32_t lines = meta[1];
    const uint32_t r0 = blockIdx.x * 256u;
    const uint32_t here = min(256u, n_rows - r0);
    const uint32_t known = r0 + 1u < lines ? min(here, lines - 1u - r0) : 0u;
    uint32_t a0 = 0u;
    if (known) {
        const uint32_t span0 = starts[r0 + 1u], span1 = min(starts[r0 + known + 1u] - 1u, n_bytes);
        a0 = span0 & ~15u;
        const uint32_t stop = min(span1, a0 + (uint32_t)STAGED_SPAN);
        for (uint32_t i = threadIdx.x; a0 + 16u * i < stop && i < (uint32_t)(STAGED_SPAN / 16); i += 256u) {
            const uint32_t pos = a0 + 16u * i;
            if (pos + 16u <= n_bytes) s_text[i] = *(const uint4 *)(text + pos);
            else
                for (uint32_t k = 0; pos + k < n_bytes; ++k) ((unsigned char *)s_text)[16u * i + k] = text[pos + k];
        }
    }
    __syncthreads();
    bool ok = false;
    const uint32_t row = r0 + threadIdx.x;
    if (threadIdx.x < here) {
        ysmr_csv::TypedRow out;
        if (threadIdx.x < known) {
            const uint32_t begin = starts[row + 1u], next = starts[row + 2u];
            if (next > begin && next - 1u <= n_bytes) {
                const StagedText at{(const unsigned char *)s_text, text, a0};
                ok = ysmr_csv::parse_line_typed(at, (long long)begin, (long long)(next - 1u), n_columns, plan, out);
            }
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < ysmr_csv::MAX_FIELDS; ++k)
                if (k < plan.n_fields) ysmr_csv::store_typed(cols.data[k], plan.type[k], (long long)row, out.bits[k]);
        }
    }
    const unsigned long long bad = __ballot(threadIdx.x < here && !ok);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(unserved, (uint32_t)__popcll(bad));
}

// The kinds of the first n_columns columns (csv_parse.h: classify_field): the same grid, staging and line-per-lane layout as the
// two parsers.  All lanes look at column `col` in the same iteration, so a column's bits are gathered by three ballots and go
// out in ONE atomic per wave and column, and only where a bit is set; OR has no order, two runs give the same words
__global__ __launch_bounds__(256) void k_csv_kinds(const unsigned char *__restrict__ text, uint32_t n_bytes, const uint32_t *__restrict__ starts,
                                                   const uint32_t *__restrict__ meta, int n_columns, uint32_t n_rows, uint32_t *__restrict__ kinds)
{
    __shared__ uint4 s_text[STAGED_SPAN / 16];
    const uint32_t lines = meta[1];
    const uint32_t r0 = blockIdx.x * 256u;
    const uint32_t here = min(256u, n_rows - r0);
    const uint32_t known = r0 + 1u < lines ? min(here, lines - 1u - r0) : 0u;
    uint32_t a0 = 0u;
    if (known) {
        const uint32_t span0 = starts[r0 + 1u], span1 = min(starts[r0 + known + 1u] - 1u, n_bytes);
        a0 = span0 & ~15u;
        const uint32_t stop = min(span1, a0 + (uint32_t)STAGED_SPAN);
        for (uint32_t i = threadIdx.x; a0 + 16u * i < stop && i < (uint32_t)(STAGED_SPAN / 16); i += 256u) {
            const uint32_t pos = a0 + 16u * i;
            if (pos + 16u <= n_bytes) s_text[i] = *(const uint4 *)(text + pos);
            else
                for (uint32_t k = 0; pos + k < n_bytes; ++k) ((unsigned char *)s_text)[16u * i + k] = text[pos + k];
        }
    }
    __syncthreads();
    const uint32_t row = r0 + threadIdx.x;
    const bool mine = threadIdx.x < here;
    bool bad = mine;                                             // (a row the index did not find, an empty line)
    long long p = 0, end = 0;
    if (threadIdx.x < known) {
        const uint32_t begin = starts[row + 1u], next = starts[row + 2u];
        if (next > begin + 1u && next - 1u <= n_bytes) { p = (long long)begin; end = (long long)(next - 1u); bad = false; }
    }
    const StagedText at{(const unsigned char *)s_text, text, a0};
    for (int col = 0; col < n_columns; ++col) {
        uint32_t bits = 0u;
        if (mine && !bad) {
            if (col) {
                if (p >= end) bad = true;                        // too few fields
                else ++p;                                        // (the ',' the field before stopped at)
            }
            if (!bad) p = ysmr_csv::classify_field(at, p, end, bits);
        }
        const bool not_int = __ballot((bits & ysmr_csv::KIND_NOT_INT) != 0u) != 0ull;
        const bool not_number = __ballot((bits & ysmr_csv::KIND_NOT_NUMBER) != 0u) != 0ull;
        const bool empty = __ballot((bits & ysmr_csv::KIND_EMPTY) != 0u) != 0ull;
        const uint32_t word = (not_int ? ysmr_csv::KIND_NOT_INT : 0u) | (not_number ? ysmr_csv::KIND_NOT_NUMBER : 0u) | (empty ? ysmr_csv::KIND_EMPTY : 0u);
        if ((threadIdx.x & 63) == 0 && word) atomicOr(&kinds[col], word);
    }
    if (mine && !bad && p != end) bad = true;                    // too many fields
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&kinds[ysmr_csv::MAX_FIELDS], ysmr_csv::KIND_BAD_LINE);
}

__global__ __launch_bounds__(256) void k_csv_keys(const uint32_t *__restrict__ id, const uint32_t *__restrict__ t, long long n,
                                                  unsigned long long *__restrict__ keys, uint32_t *__restrict__ idx)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        keys[i] = ((unsigned long long)id[i] << 32) | t[i];
        idx[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_csv_gather(const uint32_t *__restrict__ idx, long long n, ConstColumns in, Columns out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const uint32_t from = idx[i];
        out.id[i] = in.id[from];
        out.t[i] = in.t[from];
#pragma unroll
        for (int k = 0; k < 5; ++k) out.v[k][i] = in.v[k][from];
    }
}

struct HostText {
    const unsigned char *text;
    int operator()(long long i) const { return text[i]; }
};

bool wanted_of(int n_columns, const int32_t *wanted, ysmr_csv::Wanted &w)
{
    if (!wanted || n_columns < ysmr_csv::WANTED || n_columns > ysmr_csv::MAX_COLUMNS) return false;
    for (int k = 0; k < ysmr_csv::WANTED; ++k) {
        if (wanted[k] < 0 || wanted[k] >= n_columns) return false;
        for (int j = 0; j < k; ++j)
            if (wanted[j] == wanted[k]) return false;
        w.column[k] = wanted[k];
    }
    return true;
}

static_assert(csvp::MAX_COLUMNS == ysmr_csv::MAX_COLUMNS && csvp::MAX_FIELDS == ysmr_csv::MAX_FIELDS && csvp::FIELD_F64 == ysmr_csv::TYPE_F64 &&
              csvp::FIELD_EMPTY_IS_NAN == ysmr_csv::TYPED_EMPTY_IS_NAN && YSMR_CSV_EMPTY_IS_NAN == ysmr_csv::TYPED_EMPTY_IS_NAN &&
              YSMR_COL_U32 == ysmr_csv::TYPE_U32 && YSMR_COL_I64 == ysmr_csv::TYPE_I64 && YSMR_COL_I32 == ysmr_csv::TYPE_I32 &&
              YSMR_COL_I8 == ysmr_csv::TYPE_I8 && YSMR_COL_F64 == ysmr_csv::TYPE_F64, "csv_plan.h, csv_parse.h and ysmr_hip.h name the same types");

static_assert(YSMR_KIND_NOT_INT == ysmr_csv::KIND_NOT_INT && YSMR_KIND_NOT_NUMBER == ysmr_csv::KIND_NOT_NUMBER && YSMR_KIND_EMPTY == ysmr_csv::KIND_EMPTY &&
              YSMR_KIND_BAD_LINE == ysmr_csv::KIND_BAD_LINE && ysmr_csv::KIND_WORDS == 17, "csv_parse.h and ysmr_hip.h name the same kinds");

// the caller's fields -> the plan and the columns in the order of the plan; NULL, or what is wrong with them
const char *typed_plan_of(int n_columns, int n_fields, const ysmr_csv_field *fields, bool need_data, ysmr_csv::TypedPlan &plan, TypedColumns &cols)
{
    if (!fields) return "fields must be set";
    if (n_fields < 1 || n_fields > ysmr_csv::MAX_FIELDS) return "n_fields must be in 1..16 and at most n_columns";
    int32_t type[ysmr_csv::MAX_FIELDS], column[ysmr_csv::MAX_FIELDS], flags[ysmr_csv::MAX_FIELDS];
    int order[ysmr_csv::MAX_FIELDS];
    for (int k = 0; k < n_fields; ++k) { type[k] = fields[k].type; column[k] = fields[k].column; flags[k] = fields[k].flags; }
    if (const char *why = csvp::typed_fields_rule(n_columns, n_fields, type, column, flags, order)) return why;
    plan = ysmr_csv::TypedPlan{};
    cols = TypedColumns{};
    plan.n_fields = n_fields;
    for (int k = 0; k < n_fields; ++k) {
        const ysmr_csv_field &f = fields[order[k]];
        const uintptr_t align = f.type == YSMR_COL_I8 ? 1u : f.type == YSMR_COL_U32 || f.type == YSMR_COL_I32 ? 4u : 8u;
        if (need_data && (!f.data || ((uintptr_t)f.data & (align - 1u)))) return "every field's data must be set and aligned to its type";
        plan.column[k] = f.column;
        plan.type[k] = (uint8_t)f.type;
        plan.flags[k] = (uint8_t)f.flags;
        cols.data[k] = f.data;
    }
    return nullptr;
}

}  // namespace

extern "C" {

void ysmr_csv_geometry(int *index_chunk_bytes, int *rows_per_group, int *staged_span_bytes)
{
    if (index_chunk_bytes) *index_chunk_bytes = csvp::INDEX_CHUNK;
    if (rows_per_group) *rows_per_group = csvp::ROWS_PER_GROUP;
    if (staged_span_bytes) *staged_span_bytes = csvp::STAGED_SPAN;
}

size_t ysmr_csv_workspace_bytes(size_t n_bytes)
{
    csvp::Plan p;
    return csvp::plan_of(n_bytes, p) ? p.total : 0;
}

int ysmr_csv_index(void *stream, const char *text_dev, size_t n_bytes, void *workspace_dev, size_t workspace_bytes,
                   uint32_t *n_lines_dev, uint32_t *flags_dev)
{
    csvp::Plan p;
    if (!csvp::plan_of(n_bytes, p)) return ysmr::fail(YSMR_ERR_ARG, "n_bytes must be in 1..%zu, got %zu", csvp::MAX_BYTES, n_bytes);
    if (!text_dev || !workspace_dev || !n_lines_dev || !flags_dev) return ysmr::fail(YSMR_ERR_ARG, "text_dev, workspace_dev, n_lines_dev and flags_dev must be set");
    if (((uintptr_t)text_dev & 15u) || ((uintptr_t)workspace_dev & 15u)) return ysmr::fail(YSMR_ERR_ARG, "text_dev and workspace_dev must be 16-byte aligned");
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "csv workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    char *w = (char *)workspace_dev;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *counts = (uint32_t *)(w + p.counts);
    YSMR_HIP_CHECK(hipMemsetAsync(flags_dev, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_csv_index, dim3((unsigned)p.n_chunks), dim3(256), 0, st, (const unsigned char *)text_dev, (uint32_t)n_bytes,
                       (uint16_t *)(w + p.bitmap), counts, flags_dev);
    ysmr::prim::inclusive_scan_u32(st, counts, counts, p.n_chunks, (uint32_t *)(w + p.scan_temp));
    hipLaunchKernelGGL(k_csv_starts, dim3((unsigned)p.n_chunks), dim3(256), 0, st, (const unsigned char *)text_dev, (uint32_t)n_bytes,
                       (const uint16_t *)(w + p.bitmap), (const uint32_t *)counts, (uint32_t)p.n_chunks, (uint32_t *)(w + p.starts),
                       (uint32_t)p.line_capacity, (uint32_t *)(w + p.meta), n_lines_dev, flags_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_csv_parse(void *stream, const char *text_dev, size_t n_bytes, const void *workspace_dev, size_t workspace_bytes,
                   int n_columns, const int32_t *wanted, long long n_rows, uint32_t *track_id_dev, uint32_t *t_dev, double *x_dev,
                   double *y_dev, double *w_dev, double *h_dev, double *angle_dev, uint32_t *unserved_dev)
{
    csvp::Plan p;
    if (!csvp::plan_of(n_bytes, p)) return ysmr::fail(YSMR_ERR_ARG, "n_bytes must be in 1..%zu, got %zu", csvp::MAX_BYTES, n_bytes);
    ysmr_csv::Wanted wnt;
    if (!wanted_of(n_columns, wanted, wnt))
        return ysmr::fail(YSMR_ERR_ARG, "wanted must hold seven distinct positions below n_columns (7..%d), got n_columns %d", ysmr_csv::MAX_COLUMNS, n_columns);
    if (n_rows < 0 || (unsigned long long)n_rows + 2ull > p.line_capacity)
        return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..%zu for %zu bytes of text, got %lld", p.line_capacity - 2, n_bytes, n_rows);
    if (!unserved_dev) return ysmr::fail(YSMR_ERR_ARG, "unserved_dev must be set");
    hipStream_t st = (hipStream_t)stream;
    YSMR_HIP_CHECK(hipMemsetAsync(unserved_dev, 0, sizeof(uint32_t), st));
    if (n_rows == 0) return YSMR_OK;
    if (!text_dev || !workspace_dev || !track_id_dev || !t_dev || !x_dev || !y_dev || !w_dev || !h_dev || !angle_dev)
        return ysmr::fail(YSMR_ERR_ARG, "text_dev, workspace_dev and the seven columns must be set");
    if (((uintptr_t)text_dev & 15u) || ((uintptr_t)workspace_dev & 15u)) return ysmr::fail(YSMR_ERR_ARG, "text_dev and workspace_dev must be 16-byte aligned");
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "csv workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    const char *w = (const char *)workspace_dev;
    const Columns cols{track_id_dev, t_dev, {x_dev, y_dev, w_dev, h_dev, angle_dev}};
    hipLaunchKernelGGL(k_csv_parse, dim3(csvp::parse_groups(n_rows)), dim3(256), 0, st, (const unsigned char *)text_dev, (uint32_t)n_bytes,
                       (const uint32_t *)(w + p.starts), (const uint32_t *)(w + p.meta), n_columns, wnt, (uint32_t)n_rows, cols, unserved_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

size_t ysmr_csv_order_workspace_bytes(long long n_rows)
{
    csvp::OrderPlan p;
    return csvp::order_plan_of(n_rows, p) ? p.total : 0;
}

int ysmr_csv_order(void *stream, long long n_rows, const uint32_t *track_id_dev, const uint32_t *t_dev, const double *x_dev,
                   const double *y_dev, const double *w_dev, const double *h_dev, const double *angle_dev, void *workspace_dev,
                   size_t workspace_bytes, uint32_t *track_id_out, uint32_t *t_out, double *x_out, double *y_out, double *w_out,
                   double *h_out, double *angle_out)
{
    if (n_rows == 0) return YSMR_OK;
    csvp::OrderPlan p;
    if (!csvp::order_plan_of(n_rows, p)) return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..2^31-1, got %lld", n_rows);
    const void *ins[] = {track_id_dev, t_dev, x_dev, y_dev, w_dev, h_dev, angle_dev};
    void *outs[] = {track_id_out, t_out, x_out, y_out, w_out, h_out, angle_out};
    for (int k = 0; k < 7; ++k)
        if (!ins[k] || !outs[k] || ins[k] == outs[k]) return ysmr::fail(YSMR_ERR_ARG, "the seven columns and their (distinct) outputs must be set");
    if (!workspace_dev) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be set");
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "csv order workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    char *w = (char *)workspace_dev;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)std::min<long long>((n_rows + 255) / 256, 1024);
    auto *keys_a = (unsigned long long *)(w + p.keys_a), *keys_b = (unsigned long long *)(w + p.keys_b);
    auto *idx_a = (uint32_t *)(w + p.idx_a), *idx_b = (uint32_t *)(w + p.idx_b);
    hipLaunchKernelGGL(k_csv_keys, dim3(grid), dim3(256), 0, st, track_id_dev, t_dev, n_rows, keys_a, idx_a);
    const int where = ysmr::prim::radix_sort(st, keys_a, keys_b, idx_a, idx_b, (size_t)n_rows, 64, w + p.temp);
    const ConstColumns in{track_id_dev, t_dev, {x_dev, y_dev, w_dev, h_dev, angle_dev}};
    const Columns out{track_id_out, t_out, {x_out, y_out, w_out, h_out, angle_out}};
    hipLaunchKernelGGL(k_csv_gather, dim3(grid), dim3(256), 0, st, (const uint32_t *)(where ? idx_b : idx_a), n_rows, in, out);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_csv_parse_devicelike(const char *text_host, size_t n_bytes, int n_columns, const int32_t *wanted, long long row_capacity,
                              uint32_t *track_id, uint32_t *t, double *x, double *y, double *w, double *h, double *angle,
                              long long *n_rows, long long *unserved, uint32_t *flags)
{
    ysmr_csv::Wanted wnt;
    if (!wanted_of(n_columns, wanted, wnt))
        return ysmr::fail(YSMR_ERR_ARG, "wanted must hold seven distinct positions below n_columns (7..%d), got n_columns %d", ysmr_csv::MAX_COLUMNS, n_columns);
    if (!text_host || n_bytes == 0 || n_bytes > csvp::MAX_BYTES || !n_rows || !unserved || !flags || row_capacity < 0)
        return ysmr::fail(YSMR_ERR_ARG, "text_host (1..%zu bytes), n_rows, unserved and flags must be set", csvp::MAX_BYTES);
    if (row_capacity && (!track_id || !t || !x || !y || !w || !h || !angle)) return ysmr::fail(YSMR_ERR_ARG, "the seven columns must be set");
    const unsigned char *s = (const unsigned char *)text_host;
    uint32_t f = 0;
    for (size_t i = 0; i < n_bytes; ++i)
        f |= (s[i] == '"' ? ysmr_csv::FLAG_QUOTE : 0u) | (s[i] == '\r' ? ysmr_csv::FLAG_CR : 0u) | (s[i] == 0 || s[i] >= 0x80 ? ysmr_csv::FLAG_NOT_PLAIN : 0u);
    *flags = f;
    double *v[5] = {x, y, w, h, angle};
    const HostText at{s};
    long long line = 0, rows = 0, bad = 0;
    size_t begin = 0;
    while (begin < n_bytes) {
        const void *nl = std::memchr(s + begin, '\n', n_bytes - begin);
        const size_t end = nl ? (size_t)((const unsigned char *)nl - s) : n_bytes;
        if (line > 0) {
            if (rows >= row_capacity) return ysmr::fail(YSMR_ERR_CAPACITY, "more than %lld rows", row_capacity);
            ysmr_csv::Row out;
            if (ysmr_csv::parse_line(at, (long long)begin, (long long)end, n_columns, wnt, out)) {
                track_id[rows] = out.id; t[rows] = out.t;
                for (int k = 0; k < 5; ++k) v[k][rows] = out.v[k];
            } else ++bad;
            ++rows;
        }
        ++line;
        begin = end + 1;
    }
    *n_rows = rows;
    *unserved = bad;
    return YSMR_OK;
}

int ysmr_csv_parse_typed(void *stream, const char *text_dev, size_t n_bytes, const void *workspace_dev, size_t workspace_bytes,
                         int n_columns, int n_fields, const ysmr_csv_field *fields, long long n_rows, uint32_t *unserved_dev)
{
    csvp::Plan p;
    if (!csvp::plan_of(n_bytes, p)) return ysmr::fail(YSMR_ERR_ARG, "n_bytes must be in 1..%zu, got %zu", csvp::MAX_BYTES, n_bytes);
    if (n_rows < 0 || (unsigned long long)n_rows + 2ull > p.line_capacity)
        return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..%zu for %zu bytes of text, got %lld", p.line_capacity - 2, n_bytes, n_rows);
    ysmr_csv::TypedPlan plan;
    TypedColumns cols;
    if (const char *why = typed_plan_of(n_columns, n_fields, fields, n_rows > 0, plan, cols))
        return ysmr::fail(YSMR_ERR_ARG, "%s (n_columns %d, n_fields %d)", why, n_columns, n_fields);
    if (!unserved_dev) return ysmr::fail(YSMR_ERR_ARG, "unserved_dev must be set");
    hipStream_t st = (hipStream_t)stream;
    YSMR_HIP_CHECK(hipMemsetAsync(unserved_dev, 0, sizeof(uint32_t), st));
    if (n_rows == 0) return YSMR_OK;
    if (!text_dev || !workspace_dev) return ysmr::fail(YSMR_ERR_ARG, "text_dev and workspace_dev must be set");
    if (((uintptr_t)text_dev & 15u) || ((uintptr_t)workspace_dev & 15u)) return ysmr::fail(YSMR_ERR_ARG, "text_dev and workspace_dev must be 16-byte aligned");
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "csv workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    const char *w = (const char *)workspace_dev;
    hipLaunchKernelGGL(k_csv_parse_typed, dim3(csvp::parse_groups(n_rows)), dim3(256), 0, st, (const unsigned char *)text_dev, (uint32_t)n_bytes,
                       (const uint32_t *)(w + p.starts), (const uint32_t *)(w + p.meta), n_columns, plan, (uint32_t)n_rows, cols, unserved_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_csv_parse_typed_devicelike(const char *text_host, size_t n_bytes, int n_columns, int n_fields, const ysmr_csv_field *fields,
                                    long long row_capacity, long long *n_rows, long long *unserved, uint32_t *flags)
{
    if (!text_host || n_bytes == 0 || n_bytes > csvp::MAX_BYTES || !n_rows || !unserved || !flags || row_capacity < 0)
        return ysmr::fail(YSMR_ERR_ARG, "text_host (1..%zu bytes), n_rows, unserved and flags must be set", csvp::MAX_BYTES);
    ysmr_csv::TypedPlan plan;
    TypedColumns cols;
    if (const char *why = typed_plan_of(n_columns, n_fields, fields, row_capacity > 0, plan, cols))
        return ysmr::fail(YSMR_ERR_ARG, "%s (n_columns %d, n_fields %d)", why, n_columns, n_fields);
    const unsigned char *s = (const unsigned char *)text_host;
    uint32_t f = 0;
    for (size_t i = 0; i < n_bytes; ++i)
        f |= (s[i] == '"' ? ysmr_csv::FLAG_QUOTE : 0u) | (s[i] == '\r' ? ysmr_csv::FLAG_CR : 0u) | (s[i] == 0 || s[i] >= 0x80 ? ysmr_csv::FLAG_NOT_PLAIN : 0u);
    *flags = f;
    const HostText at{s};
    long long line = 0, rows = 0, bad = 0;
    size_t begin = 0;
    while (begin < n_bytes) {
        const void *nl = std::memchr(s + begin, '\n', n_bytes - begin);
        const size_t end = nl ? (size_t)((const unsigned char *)nl - s) : n_bytes;
        if (line > 0) {
            if (rows >= row_capacity) return ysmr::fail(YSMR_ERR_CAPACITY, "more than %lld rows", row_capacity);
            ysmr_csv::TypedRow out;
            if (ysmr_csv::parse_line_typed(at, (long long)begin, (long long)end, n_columns, plan, out)) {
                for (int k = 0; k < plan.n_fields; ++k) ysmr_csv::store_typed(cols.data[k], plan.type[k], rows, out.bits[k]);
            } else ++bad;
            ++rows;
        }
        ++line;
        begin = end + 1;
    }
    *n_rows = rows;
    *unserved = bad;
    return YSMR_OK;
}

int ysmr_csv_column_kinds(void *stream, const char *text_dev, size_t n_bytes, const void *workspace_dev, size_t workspace_bytes,
                          int n_columns, long long n_rows, uint32_t *kinds_dev)
{
    csvp::Plan p;
    if (!csvp::plan_of(n_bytes, p)) return ysmr::fail(YSMR_ERR_ARG, "n_bytes must be in 1..%zu, got %zu", csvp::MAX_BYTES, n_bytes);
    if (n_rows < 0 || (unsigned long long)n_rows + 2ull > p.line_capacity)
        return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..%zu for %zu bytes of text, got %lld", p.line_capacity - 2, n_bytes, n_rows);
    if (n_columns < 1 || n_columns > ysmr_csv::MAX_FIELDS) return ysmr::fail(YSMR_ERR_ARG, "n_columns must be in 1..%d, got %d", ysmr_csv::MAX_FIELDS, n_columns);
    if (!kinds_dev) return ysmr::fail(YSMR_ERR_ARG, "kinds_dev must be set");
    hipStream_t st = (hipStream_t)stream;
    YSMR_HIP_CHECK(hipMemsetAsync(kinds_dev, 0, ysmr_csv::KIND_WORDS * sizeof(uint32_t), st));
    if (n_rows == 0) return YSMR_OK;
    if (!text_dev || !workspace_dev) return ysmr::fail(YSMR_ERR_ARG, "text_dev and workspace_dev must be set");
    if (((uintptr_t)text_dev & 15u) || ((uintptr_t)workspace_dev & 15u)) return ysmr::fail(YSMR_ERR_ARG, "text_dev and workspace_dev must be 16-byte aligned");
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "csv workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    const char *w = (const char *)workspace_dev;
    hipLaunchKernelGGL(k_csv_kinds, dim3(csvp::parse_groups(n_rows)), dim3(256), 0, st, (const unsigned char *)text_dev, (uint32_t)n_bytes,
                       (const uint32_t *)(w + p.starts), (const uint32_t *)(w + p.meta), n_columns, (uint32_t)n_rows, kinds_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_csv_column_kinds_devicelike(const char *text_host, size_t n_bytes, int n_columns, uint32_t *kinds, long long *n_rows, uint32_t *flags)
{
    if (!text_host || n_bytes == 0 || n_bytes > csvp::MAX_BYTES || !kinds || !n_rows || !flags)
        return ysmr::fail(YSMR_ERR_ARG, "text_host (1..%zu bytes), kinds, n_rows and flags must be set", csvp::MAX_BYTES);
    if (n_columns < 1 || n_columns > ysmr_csv::MAX_FIELDS) return ysmr::fail(YSMR_ERR_ARG, "n_columns must be in 1..%d, got %d", ysmr_csv::MAX_FIELDS, n_columns);
    const unsigned char *s = (const unsigned char *)text_host;
    uint32_t f = 0;
    for (size_t i = 0; i < n_bytes; ++i)
        f |= (s[i] == '"' ? ysmr_csv::FLAG_QUOTE : 0u) | (s[i] == '\r' ? ysmr_csv::FLAG_CR : 0u) | (s[i] == 0 || s[i] >= 0x80 ? ysmr_csv::FLAG_NOT_PLAIN : 0u);
    *flags = f;
    for (int k = 0; k < ysmr_csv::KIND_WORDS; ++k) kinds[k] = 0u;
    const HostText at{s};
    long long line = 0, rows = 0;
    size_t begin = 0;
    while (begin < n_bytes) {
        const void *nl = std::memchr(s + begin, '\n', n_bytes - begin);
        const size_t stop = nl ? (size_t)((const unsigned char *)nl - s) : n_bytes;
        if (line > 0) {
            long long p = (long long)begin;
            const long long end = (long long)stop;
            bool bad = end <= p;
            for (int col = 0; col < n_columns && !bad; ++col) {
                if (col) {
                    if (p >= end) { bad = true; break; }
                    ++p;
                }
                uint32_t bits = 0u;
                p = ysmr_csv::classify_field(at, p, end, bits);
                kinds[col] |= bits;
            }
            if (bad || p != end) kinds[ysmr_csv::MAX_FIELDS] |= ysmr_csv::KIND_BAD_LINE;
            ++rows;
        }
        ++line;
        begin = stop + 1;
    }
    *n_rows = rows;
    return YSMR_OK;
}

}  // extern "C"
