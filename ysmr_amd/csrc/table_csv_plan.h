// table_csv_plan.h -- the host-only part of table_csv.hip: the geometry of the writing kernels, the widths of the fields, the
// bound of the text and the layout of the workspace, with what they refuse.  Plain C++ with no HIP in it, so that
// tests/table_plan_check.cc compiles it alone, under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tablep {

constexpr int COL_U32 = 0, COL_I64 = 1, COL_I32 = 2, COL_I8 = 3, COL_F64 = 4, N_TYPES = 5;
constexpr int MAX_COLUMNS = 16;
// the widest field of each type: 4294967295, -9223372036854775808, -2147483648, -128, -1.2345678901234567e-308
constexpr int FIELD_WIDTH[N_TYPES] = {10, 20, 11, 4, 24};

// ---- geometry (ysmr_table_format_geometry reports it) -----------------------------------------------------------------------
constexpr int ROWS_PER_GROUP = 128;                                  // a row per lane, two waves
constexpr int MAX_ROW_BYTES = MAX_COLUMNS * (FIELD_WIDTH[COL_F64] + 1);   // sixteen float64 fields with their separators: 400
// The staging is sized for the worst case of the DECLARED column types: ROWS_PER_GROUP rows of row_stride bytes each, dynamic
// LDS.  This is its largest value (sixteen float64 columns); the selected table's is 21504, the analysed table's 32256.
constexpr int STAGED_BYTES = ROWS_PER_GROUP * MAX_ROW_BYTES;         // 51200
constexpr int WIDE_SLOT = 24;                                        // bytes of a wide cell's side slot
constexpr int SCAN_TILE = 2048;                                      // prim.h: the tile of its prefix sum (table_csv.hip asserts it)
// byte offsets and counts are 32-bit numbers in the scans
constexpr size_t MAX_TEXT = 0xFFFFFFFFull;

struct Plan {
    int row_bytes;          // the longest row the declared types can give (csv: the sum of (width + 1) over the columns)
    int row_stride;         // ... rounded up to 4: a row's place in the staging
    int n_f64;              // float64 columns: those that may hold wide cells
    size_t groups;          // workgroups of the row printer = pieces
    size_t piece_stride;    // bytes between two pieces in the workspace (a multiple of 16, with 16 bytes of slack behind the text)
    size_t suffix, wide_incl, wide_temp, wide_slots, wide_len, piece_len, piece_incl, piece_temp, pieces, total;   // layout_of
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

// false: a column count outside 1 .. 16 or an unknown type
inline bool row_of(int n_columns, const int32_t *types, int &row_bytes, int &n_f64)
{
    row_bytes = 0; n_f64 = 0;
    if (n_columns < 1 || n_columns > MAX_COLUMNS || !types) return false;
    for (int c = 0; c < n_columns; ++c) {
        if (types[c] < 0 || types[c] >= N_TYPES) return false;
        row_bytes += FIELD_WIDTH[types[c]] + 1;
        n_f64 += types[c] == COL_F64;
    }
    return true;
}

// the header plus n_rows longest lines; false: a negative count, arithmetic beyond size_t, or more than the 32-bit scans hold
inline bool bound_of(long long n_rows, int row_bytes, size_t header_bytes, size_t &bound)
{
    bound = 0;
    if (n_rows < 0 || row_bytes <= 0) return false;
    size_t text, all;
    if ((unsigned long long)n_rows > SIZE_MAX || __builtin_mul_overflow((size_t)n_rows, (size_t)row_bytes, &text) ||
        __builtin_add_overflow(text, header_bytes, &all) || all > MAX_TEXT)
        return false;
    bound = all;
    return true;
}

// The workspace's areas, one layout for the two printers: `suffix` (suffix_area bytes: table_csv.hip has none, xlsx.hip keeps
// its sheet's end there), the wide cells' counts, scan words, slots and lengths, the pieces' lengths, sums and scan words, the
// pieces.  n rows of n_f64 float64 columns whose text fits MAX_TEXT (so n * n_f64 is far from overflow); n = 0 is served and
// has the suffix area alone.  false: a size beyond size_t
inline bool layout_of(size_t n, int n_f64, size_t groups, size_t piece_stride, size_t suffix_area, Plan &p)
{
    size_t at = 0;
    bool fits = true;
    auto take = [&](size_t count, size_t each) {
        const size_t here = at;
        size_t bytes;
        if (__builtin_mul_overflow(count, each, &bytes) || bytes > SIZE_MAX - 255 || __builtin_add_overflow(at, align256(bytes), &at)) fits = false;
        return here;
    };
    // (every float64 cell may be a wide one, and the host is not asked in between: the side slots are sized for that)
    const bool wide = n_f64 && n;
    const size_t cells = n * (size_t)n_f64;
    p.suffix = take(suffix_area, 1);
    p.wide_incl = take(wide ? n : 0, sizeof(uint32_t));                  // wide cells per row, then their inclusive sums
    p.wide_temp = take(wide ? scan_words(n) : 0, sizeof(uint32_t));
    p.wide_slots = take(cells, WIDE_SLOT);
    p.wide_len = take(cells, 1);
    p.piece_len = take(groups, sizeof(uint32_t));
    p.piece_incl = take(groups, sizeof(uint32_t));
    p.piece_temp = take(n ? scan_words(groups) : 0, sizeof(uint32_t));
    p.pieces = take(groups, piece_stride);
    p.total = at;
    return fits;
}

// the workspace of n_rows > 0 rows (n_rows = 0 needs none); false as bound_of with no header
inline bool plan_of(long long n_rows, int n_columns, const int32_t *types, Plan &p)
{
    size_t text;
    if (!row_of(n_columns, types, p.row_bytes, p.n_f64) || n_rows <= 0 || !bound_of(n_rows, p.row_bytes, 0, text)) return false;
    const size_t n = (size_t)n_rows;
    p.row_stride = (p.row_bytes + 3) / 4 * 4;
    p.groups = (n + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP;
    p.piece_stride = ((size_t)ROWS_PER_GROUP * (size_t)p.row_bytes + 15) / 16 * 16 + 16;
    return layout_of(n, p.n_f64, p.groups, p.piece_stride, 0, p);
}

}  // namespace tablep
