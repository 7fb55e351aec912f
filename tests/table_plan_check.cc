// Stand-alone check of the host-only part of the device csv writer (ysmr_amd/csrc/table_csv_plan.h), of the wide float printer
// (ysmr_amd/csrc/fmt.h: shortest_wide) and of the row printer's host form (ysmr_amd/csrc/table_csv_row.h), meant to be built with
// the host's address and undefined-behaviour sanitizers (tests/test_table_plan_sanitized.py builds and runs it).  It walks row
// counts and column sets up to the refused limits and compares the bound and every workspace part with the same sum worked out in
// 128 bits; it prints wide cells into heap blocks of exactly 24 bytes and rows of all-widest fields into heap blocks of exactly
// the bound, so that a byte beyond either is an error the sanitizer reports.  Prints "ok <cases>" and returns 0, or says what failed.
#include "table_csv_plan.h"
#include "table_csv_row.h"

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

int main()
{
    long cases = 0;
    // ---- the bound and the workspace ----
    const std::vector<std::vector<int32_t>> sets = {
        {4}, {0}, {3}, {1, 0, 0, 4, 4, 4, 4, 4}, {0, 0, 4, 4, 4, 4, 4, 2, 3, 3, 4, 4, 3}, std::vector<int32_t>(16, 4), std::vector<int32_t>(16, 3),
        {0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 1}};
    const std::vector<long long> counts = {LLONG_MIN, -1, 0, 1, 2, 127, 128, 129, 2047, 2048, 2049, 262145, 1000003, 10737418, 10737419, 42949672,
                                           42949673, 171798691, 171798692, 858993459, 858993460, 1ll << 31, 1ll << 32, 1ll << 40, LLONG_MAX};
    const std::vector<unsigned long long> headers = {0, 1, 77, 300, 0xFFFFFFFFull, 1ull << 32, (unsigned long long)SIZE_MAX - 1,
                                                     (unsigned long long)SIZE_MAX};
    for (const auto &types : sets) {
        int row_bytes = 0, n_f64 = 0, line = 0, f64 = 0;
        for (int32_t t : types) { line += WIDTH[t] + 1; f64 += t == 4; }
        if (!tablep::row_of((int)types.size(), types.data(), row_bytes, n_f64) || row_bytes != line || n_f64 != f64) {
            std::printf("row_of: %d bytes, %d float64 columns, expected %d, %d\n", row_bytes, n_f64, line, f64);
            return 1;
        }
        for (long long n : counts) {
            for (unsigned long long head : headers) {
                ++cases;
                size_t bound = 1;
                const bool ok = tablep::bound_of(n, row_bytes, (size_t)head, bound);
                const u128 want = n < 0 ? 0 : (u128)n * (u128)line + head;
                const bool valid = n >= 0 && want <= 0xFFFFFFFFull;
                if (ok != valid || (ok ? (u128)bound != want : bound != 0)) {
                    std::printf("bound_of(%lld rows of %d, header %llu): %s, %zu\n", n, line, head, ok ? "accepted" : "refused", bound);
                    return 1;
                }
            }
            ++cases;
            tablep::Plan p = {};
            const bool ok = tablep::plan_of(n, (int)types.size(), types.data(), p);
            const bool valid = n > 0 && (u128)n * (u128)line <= 0xFFFFFFFFull;
            if (ok != valid) { std::printf("plan_of(%lld rows of %d): %s\n", n, line, ok ? "accepted" : "refused"); return 1; }
            if (!ok) continue;
            const u128 rows = (u128)n, groups = (rows + 127) / 128, stride = ((u128)128 * line + 15) / 16 * 16 + 16, cells = rows * f64;
            const u128 want = up(f64 ? rows * 4 : 0) + up(f64 ? scan_words(rows) * 4 : 0) + up(cells * 24) + up(cells) + up(groups * 4) + up(groups * 4) +
                              up(scan_words(groups) * 4) + up(groups * stride);
            if ((u128)p.total != want || p.total % 256 || (u128)p.groups != groups || (u128)p.piece_stride != stride || p.row_stride % 4 ||
                p.row_stride < line || p.row_stride >= line + 4 || tablep::ROWS_PER_GROUP * p.row_stride > tablep::STAGED_BYTES ||
                !(p.wide_incl <= p.wide_temp && p.wide_temp <= p.wide_slots && p.wide_slots <= p.wide_len && p.wide_len <= p.piece_len &&
                  p.piece_len < p.piece_incl && p.piece_incl < p.piece_temp && p.piece_temp < p.pieces && p.pieces < p.total) ||
                p.wide_len - p.wide_slots < (size_t)cells * 24 || p.piece_len - p.wide_len < (size_t)cells || p.total - p.pieces < (size_t)(groups * stride) ||
                p.pieces % 16 || p.piece_stride % 16) {
                std::printf("plan_of(%lld rows of %d): total %zu, expected %.0Lf\n", n, line, p.total, (long double)want);
                return 1;
            }
        }
    }
    {
        int row_bytes = 0, n_f64 = 0;
        const int32_t bad_type[2] = {4, 5}, negative[1] = {-1};
        tablep::Plan p = {};
        ++cases;
        if (tablep::row_of(0, bad_type, row_bytes, n_f64) || tablep::row_of(17, bad_type, row_bytes, n_f64) || tablep::row_of(2, bad_type, row_bytes, n_f64) ||
            tablep::row_of(1, negative, row_bytes, n_f64) || tablep::row_of(1, nullptr, row_bytes, n_f64) || tablep::plan_of(5, 2, bad_type, p)) {
            std::printf("a column set that must be refused was accepted\n");
            return 1;
        }
    }
    // ---- the wide printer: a cell into a heap block of exactly 24 bytes ----
    {
        std::vector<double> values = {5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308, 1.5e-13, 1e-14, 1e300,
                                      1.2345678901234567e-308, 1e23, 9007199254740993.0, 1.2345678901234568e17, 16777216.0, 9.5367431640625e-07};
        unsigned long long state = 0x9E3779B97F4A7C15ull;
        for (int k = 0; k < 4000; ++k) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const double v = ysmr_fmt::double_of(state >> 1);
            if (v == v && v != 0 && v <= 1.7976931348623157e308) values.push_back(v);
        }
        for (double v : values) {
            for (int sign = 0; sign < 2; ++sign) {
                ++cases;
                const double x = sign ? -v : v;
                char *block = (char *)std::malloc(tablep::WIDE_SLOT);
                char *end = ysmr_fmt::put_f64_wide(block, x);
                const std::string got(block, end);
                std::free(block);
                // (the text reads back as the value, with no more than the 17 digits that always do)
                size_t digits = 0;
                for (size_t i = 0; i < got.size() && got[i] != 'e'; ++i) digits += got[i] >= '0' && got[i] <= '9';
                if (std::strtod(got.c_str(), nullptr) != x || digits > 17 + 5 || got.size() > (size_t)tablep::WIDE_SLOT) {
                    std::printf("wide printer: %a -> %s\n", x, got.c_str());
                    return 1;
                }
            }
        }
        char *block = (char *)std::malloc(tablep::WIDE_SLOT);
        const std::string widest(block, ysmr_fmt::put_f64_wide(block, -1.2345678901234567e-308));
        std::free(block);
        if (widest != "-1.2345678901234567e-308" || widest.size() != (size_t)tablep::WIDE_SLOT) { std::printf("widest cell: %s\n", widest.c_str()); return 1; }
    }
    // ---- the row printer: rows of all-widest fields into a heap block of exactly the bound ----
    for (const auto &types : sets) {
        const int n_columns = (int)types.size();
        const long long n = 37;
        std::vector<std::vector<unsigned char>> store((size_t)n_columns);
        const void *data[tablep::MAX_COLUMNS];
        std::string line;
        for (int c = 0; c < n_columns; ++c) {
            const uint32_t u32 = 4294967295u; const int64_t i64 = INT64_MIN; const int32_t i32 = INT32_MIN; const int8_t i8 = -128;
            const double f64 = -1.2345678901234567e-308;
            const void *src[5] = {&u32, &i64, &i32, &i8, &f64};
            const size_t each[5] = {4, 8, 4, 1, 8};
            const char *text[5] = {"4294967295", "-9223372036854775808", "-2147483648", "-128", "-1.2345678901234567e-308"};
            store[(size_t)c].resize(each[types[c]] * (size_t)n);                 // (exactly the column: row n is out of bounds)
            for (long long r = 0; r < n; ++r) std::memcpy(store[(size_t)c].data() + each[types[c]] * (size_t)r, src[types[c]], each[types[c]]);
            data[c] = store[(size_t)c].data();
            line += text[types[c]];
            line += c + 1 < n_columns ? ',' : '\n';
        }
        int row_bytes = 0, n_f64 = 0;
        size_t bound = 0;
        tablep::row_of(n_columns, types.data(), row_bytes, n_f64);
        tablep::bound_of(n, row_bytes, 0, bound);
        char *block = (char *)std::malloc(bound);
        char *p = block;
        long long wide = 0;
        for (long long r = 0; r < n; ++r) p = tablep::put_row(p, n_columns, types.data(), data, r, &wide);
        std::string expect;
        for (long long r = 0; r < n; ++r) expect += line;
        const size_t used = (size_t)(p - block);
        const bool same = used == bound && expect.size() == bound && std::memcmp(block, expect.data(), bound) == 0;
        std::free(block);
        ++cases;
        if (!same || wide != n * n_f64) { std::printf("rows of %d widest fields: %zu bytes, %lld wide cells\n", n_columns, used, wide); return 1; }
    }
    // a NaN alone on its line
    {
        const double nan = ysmr_fmt::double_of(0x7FF8000000000000ull);
        const int32_t type = 4;
        const void *data[1] = {&nan};
        char *block = (char *)std::malloc(25);
        long long wide = 0;
        const std::string got(block, tablep::put_row(block, 1, &type, data, 0, &wide));
        std::free(block);
        ++cases;
        if (got != "\"\"\n" || wide) { std::printf("a NaN alone: %s\n", got.c_str()); return 1; }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
