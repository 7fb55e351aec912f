// Stand-alone check of the host-only part of the worksheet printer (ysmr_amd/csrc/xlsx_plan.h) and of the row printer's host form
// (ysmr_amd/csrc/xlsx_row.h), meant to be built with the host's address and undefined-behaviour sanitizers
// (tests/test_xlsx_plan_sanitized.py builds and runs it).  It walks row counts, first rows and column sets up to the refused limits
// and compares the longest row, the bound and every workspace part with the same sums worked out in 128 bits; it prints rows of
// all-widest cells into heap blocks of exactly the plan's row size -- at the sheet's last rows, where every number has its most
// digits -- so that a byte beyond is an error the sanitizer reports.  Prints "ok <cases>" and returns 0, or says what failed.
#include "xlsx_plan.h"
#include "xlsx_row.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef unsigned __int128 u128;

static u128 up(u128 v) { return (v + 255) / 256 * 256; }

static u128 scan_words(u128 n)
{
    u128 words = 0;
    while (n > 2048) { n = (n + 2047) / 2048; words += (n + 63) / 64 * 64; }
    return words + 64;
}

static const int WIDTH[5] = {10, 20, 11, 4, 24};

static int digits(long long v) { return (int)std::to_string(v).size(); }

int main()
{
    long cases = 0;
    const std::vector<std::vector<int32_t>> sets = {
        {4}, {0}, {3}, {1, 0, 0, 4, 4, 4, 4, 4}, {0, 0, 4, 4, 4, 4, 4, 2, 3, 3, 4, 4, 3}, std::vector<int32_t>(16, 4), std::vector<int32_t>(16, 3),
        {0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 1}};
    const std::vector<long long> counts = {LLONG_MIN, -1, 0, 1, 2, 7, 10, 11, 63, 64, 65, 2048, 2049, 131073, 999999, 1000000, 1000001, 1048569, 1048570,
                                           1048575, 1048576, 1048577, 1ll << 31, LLONG_MAX};
    const std::vector<long long> firsts = {LLONG_MIN, -1, 0, 1, 2, 9, 10, 99, 1000, 1048570, 1048576, 1048577, LLONG_MAX};
    const std::vector<unsigned long long> extras = {0, 1, 24, 300, 0xFFFFFFFFull, 1ull << 32, (unsigned long long)SIZE_MAX};
    // ---- the longest row, the bound and the workspace ----
    for (const auto &types : sets) {
        const int n_columns = (int)types.size();
        for (int with_index = 0; with_index < 2; ++with_index) {
            for (long long n : counts) {
                for (long long first : firsts) {
                    ++cases;
                    const bool inside = n >= 0 && first >= 1 && first <= 1048576 && (u128)first + (u128)n <= (u128)1048577;
                    int row_bytes = -1, n_f64 = -1;
                    const bool ok = xlsxp::row_of(n_columns, types.data(), with_index != 0, n, first, row_bytes, n_f64);
                    if (ok != inside) { std::printf("row_of(%lld rows from %lld): %s\n", n, first, ok ? "accepted" : "refused"); return 1; }
                    if (!ok) {
                        size_t bound = 1;
                        xlsxp::Plan p = {};
                        if (xlsxp::bound_of(n, first, 100, 0, 0, bound) || bound != 0 || xlsxp::plan_of(n, first, n_columns, types.data(), with_index != 0, 24, p)) {
                            std::printf("bound_of / plan_of(%lld rows from %lld) accepted\n", n, first);
                            return 1;
                        }
                        continue;
                    }
                    const int rd = digits(first + (n ? n - 1 : 0)), id = digits(n ? n - 1 : 0);
                    int line = 8 + rd + 2 + 6 + (with_index ? 7 + rd + 11 + id + 8 : 0), f64 = 0;
                    for (int32_t t : types) { line += 6 + 1 + rd + 5 + WIDTH[t] + 8; f64 += t == 4; }
                    if (row_bytes != line || n_f64 != f64 || row_bytes > xlsxp::MAX_ROW_BYTES) {
                        std::printf("row_of(%lld rows from %lld): %d bytes, %d float64 columns, expected %d, %d\n", n, first, row_bytes, n_f64, line, f64);
                        return 1;
                    }
                    for (unsigned long long prefix : extras) {
                        for (unsigned long long suffix : extras) {
                            ++cases;
                            size_t bound = 1;
                            const bool fits = xlsxp::bound_of(n, first, row_bytes, (size_t)prefix, (size_t)suffix, bound);
                            const u128 want = (u128)n * (u128)line + prefix + suffix;
                            if (fits != (want <= 0xFFFFFFFFull) || (fits ? (u128)bound != want : bound != 0)) {
                                std::printf("bound_of(%lld rows of %d, %llu, %llu): %s, %zu\n", n, line, prefix, suffix, fits ? "accepted" : "refused", bound);
                                return 1;
                            }
                        }
                    }
                    const size_t suffix = 24;
                    xlsxp::Plan p = {};
                    if (!xlsxp::plan_of(n, first, n_columns, types.data(), with_index != 0, suffix, p)) { std::printf("plan_of(%lld rows from %lld) refused\n", n, first); return 1; }
                    const u128 rows = (u128)n, groups = (rows + 63) / 64, stride = ((u128)64 * line + 15) / 16 * 16 + 16, cells = rows * f64;
                    const bool wide = f64 && n;
                    const u128 want = up(suffix + 1) + up(wide ? rows * 4 : 0) + up(wide ? scan_words(rows) * 4 : 0) + up(cells * 24) + up(cells) + up(groups * 4) +
                                      up(groups * 4) + up(n ? scan_words(groups) * 4 : 0) + up(groups * stride);
                    if ((u128)p.total != want || p.total % 256 || (u128)p.groups != groups || (u128)p.piece_stride != stride || p.row_stride % 4 ||
                        p.row_stride < line || p.row_stride >= line + 4 || xlsxp::ROWS_PER_GROUP * p.row_stride > xlsxp::STAGED_BYTES ||
                        !(p.suffix < p.wide_incl && p.wide_incl <= p.wide_temp && p.wide_temp <= p.wide_slots && p.wide_slots <= p.wide_len &&
                          p.wide_len <= p.piece_len && p.piece_len <= p.piece_incl && p.piece_incl <= p.piece_temp && p.piece_temp <= p.pieces &&
                          p.pieces <= p.total) ||
                        p.wide_incl - p.suffix < suffix || p.wide_len - p.wide_slots < (size_t)cells * 24 || p.piece_len - p.wide_len < (size_t)cells ||
                        p.total - p.pieces < (size_t)(groups * stride) || p.pieces % 16 || p.piece_stride % 16 || p.suffix % 16) {
                        std::printf("plan_of(%lld rows from %lld of %d): total %zu, expected %.0Lf\n", n, first, line, p.total, (long double)want);
                        return 1;
                    }
                }
            }
        }
    }
    {
        int row_bytes = 0, n_f64 = 0;
        const int32_t bad_type[2] = {4, 5}, negative[1] = {-1};
        xlsxp::Plan p = {};
        ++cases;
        if (xlsxp::row_of(0, bad_type, true, 1, 2, row_bytes, n_f64) || xlsxp::row_of(17, bad_type, true, 1, 2, row_bytes, n_f64) ||
            xlsxp::row_of(2, bad_type, true, 1, 2, row_bytes, n_f64) || xlsxp::row_of(1, negative, true, 1, 2, row_bytes, n_f64) ||
            xlsxp::row_of(1, nullptr, true, 1, 2, row_bytes, n_f64) || xlsxp::plan_of(5, 2, 2, bad_type, true, 0, p)) {
            std::printf("a column set that must be refused was accepted\n");
            return 1;
        }
        if (xlsxp::MAX_ROW_BYTES != 879 || xlsxp::STAGED_BYTES != 64 * 880) { std::printf("geometry: %d, %d\n", xlsxp::MAX_ROW_BYTES, xlsxp::STAGED_BYTES); return 1; }
    }
    // ---- the row printer: rows of all-widest cells into a heap block of exactly the plan's row size ----
    // (n rows that END at the sheet's last row; the full sheet of 2^20 rows has the longest row numbers too: its last three rows)
    for (const auto &types : sets) {
        const int n_columns = (int)types.size();
        for (int with_index = 0; with_index < 2; ++with_index) {
            for (long long n : {1ll, 7ll, 37ll, 1048576ll}) {
                const long long first = 1048576 - n + 1, from = n > 3 ? n - 3 : 0;
                std::vector<std::vector<unsigned char>> store((size_t)n_columns);
                const void *data[xlsxp::MAX_COLUMNS];
                const uint32_t u32 = 4294967295u; const int64_t i64 = INT64_MIN; const int32_t i32 = INT32_MIN; const int8_t i8 = -128;
                const double f64 = -1.2345678901234567e-308;
                const void *src[5] = {&u32, &i64, &i32, &i8, &f64};
                const size_t each[5] = {4, 8, 4, 1, 8};
                const char *text[5] = {"4294967295", "-9223372036854775808", "-2147483648", "-128", "-1.2345678901234567e-308"};
                for (int c = 0; c < n_columns; ++c) {
                    const size_t size = each[types[c]];
                    store[(size_t)c].resize(size * (size_t)n);                       // (exactly the column: row n is out of bounds)
                    for (long long r = from; r < n; ++r) std::memcpy(store[(size_t)c].data() + size * (size_t)r, src[types[c]], size);
                    data[c] = store[(size_t)c].data();
                }
                int row_bytes = 0, n_f64 = 0;
                xlsxp::row_of(n_columns, types.data(), with_index != 0, n, first, row_bytes, n_f64);
                long long wide = 0;
                for (long long r = from; r < n; ++r) {
                    char *block = (char *)std::malloc((size_t)row_bytes);
                    const std::string got(block, xlsxp::put_row(block, n_columns, types.data(), data, r, first, with_index != 0, &wide));
                    std::free(block);
                    const std::string row = std::to_string(first + r);
                    std::string expect = "<row r=\"" + row + "\">";
                    if (with_index) expect += "<c r=\"A" + row + "\" s=\"1\"><v>" + std::to_string(r) + "</v></c>";
                    for (int c = 0; c < n_columns; ++c)
                        expect += std::string("<c r=\"") + (char)('A' + c + with_index) + row + "\"><v>" + text[types[c]] + "</v></c>";
                    expect += "</row>";
                    ++cases;
                    // (the last row has every number at its most digits: it fills the block exactly)
                    if (got != expect || got.size() > (size_t)row_bytes || (r == n - 1 && got.size() != (size_t)row_bytes)) {
                        std::printf("row %lld of %lld from %lld, %d columns: %zu bytes of %d\n%s\n", r, n, first, n_columns, got.size(), row_bytes, got.c_str());
                        return 1;
                    }
                }
                if (wide != (n - from) * n_f64) { std::printf("wide cells: %lld\n", wide); return 1; }
            }
        }
    }
    // a row of only NaN, both infinities, a zero: into a block of exactly the row size
    {
        const double nan = ysmr_fmt::double_of(0x7FF8000000000000ull), inf = ysmr_fmt::double_of(0x7FF0000000000000ull), zero = -0.0;
        const int32_t types[3] = {4, 4, 4};
        int row_bytes = 0, n_f64 = 0;
        xlsxp::row_of(3, types, true, 1, 7, row_bytes, n_f64);
        long long wide = 0;
        const void *nans[3] = {&nan, &nan, &nan};
        char *block = (char *)std::malloc((size_t)row_bytes);
        const std::string empty(block, xlsxp::put_row(block, 3, types, nans, 0, 7, true, &wide));
        const std::string bare(block, xlsxp::put_row(block, 3, types, nans, 0, 7, false, &wide));
        const double minus = -inf;
        const void *mixed[3] = {&inf, &minus, &zero};
        const std::string other(block, xlsxp::put_row(block, 3, types, mixed, 0, 7, true, &wide));
        std::free(block);
        ++cases;
        if (empty != "<row r=\"7\"><c r=\"A7\" s=\"1\"><v>0</v></c></row>" || bare != "<row r=\"7\"></row>" || wide ||
            other != "<row r=\"7\"><c r=\"A7\" s=\"1\"><v>0</v></c><c r=\"B7\" t=\"str\"><v>inf</v></c><c r=\"C7\" t=\"str\"><v>-inf</v></c>"
                     "<c r=\"D7\"><v>-0.0</v></c></row>" || other.size() > (size_t)row_bytes) {
            std::printf("special rows:\n%s\n%s\n%s\n", empty.c_str(), bare.c_str(), other.c_str());
            return 1;
        }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
