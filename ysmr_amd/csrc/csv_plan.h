// csv_plan.h -- the host-only part of csv.hip: the geometry of the reading kernels, the argument rules and the layout of the
// workspaces.  Plain C++ with no HIP in it, so that tests/csv_plan_check.cc compiles it alone, under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace csvp {

// ---- geometry (ysmr_csv_geometry reports it) -------------------------------------------------------------------------------
constexpr int LOAD_BYTES = 16;                               // one lane's load of the index pass
constexpr int INDEX_ROUNDS = 4;                              // loads per lane
constexpr int INDEX_CHUNK = 256 * LOAD_BYTES * INDEX_ROUNDS; // bytes of text per workgroup of the index pass
constexpr int ROWS_PER_GROUP = 256;                          // a line per lane of the parse
constexpr int STAGED_SPAN = 40960;                           // bytes of a workgroup's lines held in LDS, from a 16-byte boundary
constexpr int SCAN_TILE = 2048;                              // prim.h: the tile of its prefix sum (csv.hip asserts the two agree)
// A served line holds seven wanted fields of a byte at least, six commas and its '\n': a file with more lines than
// n_bytes / MIN_LINE_BYTES + 2 holds a line that is not served, and the table of line starts need not be larger
constexpr int MIN_LINE_BYTES = 14;
// byte offsets are 32-bit numbers in the kernels, with room for the end mark n_bytes + 1
constexpr size_t MAX_BYTES = 0x7FFFFF00u;
constexpr long long MAX_ROWS = 0x7FFFFFFFll;

struct Plan {
    size_t n_chunks;                  // workgroups of the index pass
    size_t line_capacity;             // entries of `starts`: line L is [starts[L], starts[L + 1] - 1)
    size_t meta, bitmap, counts, scan_temp, starts, total;
};

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// u32 words the prefix sum over n values needs (prim.h: scan_temp_words, restated without HIP)
inline size_t scan_words(size_t n)
{
    size_t words = 0;
    while (n > (size_t)SCAN_TILE) {
        n = (n + SCAN_TILE - 1) / SCAN_TILE;
        words += (n + 63) / 64 * 64;
    }
    return words + 64;
}

// false: nothing to read, or more than the kernels' 32-bit offsets hold (every term below then fits a size_t of 64 bits;
// with a narrower size_t the sums are checked)
inline bool plan_of(size_t n_bytes, Plan &p)
{
    if (n_bytes == 0 || n_bytes > MAX_BYTES) return false;
    p.n_chunks = (n_bytes + INDEX_CHUNK - 1) / INDEX_CHUNK;
    p.line_capacity = n_bytes / MIN_LINE_BYTES + 3;
    size_t at = 0;
    bool fits = true;
    auto take = [&](size_t count, size_t each) {
        const size_t here = at;
        size_t bytes;
        if (__builtin_mul_overflow(count, each, &bytes) || bytes > SIZE_MAX - 255 || __builtin_add_overflow(at, align256(bytes), &at)) fits = false;
        return here;
    };
    p.meta = take(64, sizeof(uint32_t));                                   // newlines, lines, flags
    p.bitmap = take(p.n_chunks * (INDEX_CHUNK / LOAD_BYTES), sizeof(uint16_t));   // a bit per byte: it is a '\n'
    p.counts = take(p.n_chunks, sizeof(uint32_t));                         // newlines per chunk, then their inclusive sums
    p.scan_temp = take(scan_words(p.n_chunks), sizeof(uint32_t));
    p.starts = take(p.line_capacity, sizeof(uint32_t));
    p.total = at;
    return fits;
}

// ---- ordering: keys, row numbers, both twice, and the radix passes' histograms --------------------------------------------
constexpr int RADIX_TILE = 2048;      // prim.h (asserted in csv.hip)

struct OrderPlan { size_t keys_a, keys_b, idx_a, idx_b, temp, total; };

inline bool order_plan_of(long long n_rows, OrderPlan &p)
{
    if (n_rows <= 0 || n_rows > MAX_ROWS) return false;
    const size_t n = (size_t)n_rows;
    size_t at = 0;
    bool fits = true;
    auto take = [&](size_t count, size_t each) {
        const size_t here = at;
        size_t bytes;
        if (__builtin_mul_overflow(count, each, &bytes) || bytes > SIZE_MAX - 255 || __builtin_add_overflow(at, align256(bytes), &at)) fits = false;
        return here;
    };
    p.keys_a = take(n, sizeof(uint64_t));
    p.keys_b = take(n, sizeof(uint64_t));
    p.idx_a = take(n, sizeof(uint32_t));
    p.idx_b = take(n, sizeof(uint32_t));
    const size_t cells = 256 * ((n + RADIX_TILE - 1) / RADIX_TILE);
    p.temp = take((cells + 63) / 64 * 64 + scan_words(cells), sizeof(uint32_t));
    p.total = at;
    return fits;
}

// ---- the typed parse: the rules of its field list ----------------------------------------------------------------------------
constexpr int MAX_COLUMNS = 4096, MAX_FIELDS = 16, FIELD_TYPES = 5, FIELD_F64 = 4, FIELD_EMPTY_IS_NAN = 1;   // (csv.hip asserts them)

// NULL and order[0 .. n_fields): the fields by ascending column -- or what is wrong with the list.  type / column / flags: one
// entry per field.
inline const char *typed_fields_rule(int n_columns, int n_fields, const int32_t *type, const int32_t *column, const int32_t *flags,
                                     int *order)
{
    if (n_columns < 1 || n_columns > MAX_COLUMNS) return "n_columns must be in 1..4096";
    if (n_fields < 1 || n_fields > MAX_FIELDS || n_fields > n_columns) return "n_fields must be in 1..16 and at most n_columns";
    for (int k = 0; k < n_fields; ++k) {
        if (type[k] < 0 || type[k] >= FIELD_TYPES) return "a field's type must be one of YSMR_COL_U32 / I64 / I32 / I8 / F64";
        if (column[k] < 0 || column[k] >= n_columns) return "a field's column must be below n_columns";
        if ((flags[k] & ~FIELD_EMPTY_IS_NAN) || (flags[k] && type[k] != FIELD_F64)) return "a field's flags: YSMR_CSV_EMPTY_IS_NAN, on YSMR_COL_F64 only";
        int at = k;                                   // insertion by column
        for (; at > 0 && column[order[at - 1]] > column[k]; --at) order[at] = order[at - 1];
        if (at > 0 && column[order[at - 1]] == column[k]) return "the fields' columns must be distinct";
        order[at] = k;
    }
    return nullptr;
}

// the grid of the parse: a workgroup per ROWS_PER_GROUP lines
inline unsigned parse_groups(long long n_rows) { return (unsigned)((n_rows + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP); }

}  // namespace csvp
