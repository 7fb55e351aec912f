// Stand-alone check of the host-only part of the device csv reader (ysmr_amd/csrc/csv_plan.h) and of the line parser's host form
// (ysmr_amd/csrc/csv_parse.h), meant to be built with the host's address and undefined-behaviour sanitizers
// (tests/test_csv_plan_sanitized.py builds and runs it).  It walks text sizes and row counts, the limits among them, and compares
// every workspace part with the same sum worked out in 128 bits; and it parses lines that sit in heap blocks of exactly their
// size, so that a fetch beyond a line's end is an error the sanitizer reports.  Prints "ok <cases>" and returns 0, or says what
// failed.
#include "csv_plan.h"
#include "csv_parse.h"

#include <climits>
#include <cmath>
#include <cstdio>
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

struct HeapText {
    const unsigned char *text;
    int operator()(long long i) const { return text[i]; }
};

static bool parse(const std::string &line, int n_columns, const ysmr_csv::Wanted &w, ysmr_csv::Row &row)
{
    std::vector<unsigned char> block(line.begin(), line.end());      // exactly the line: one byte more is out of bounds
    const HeapText at{block.data()};
    return ysmr_csv::parse_line(at, 0, (long long)block.size(), n_columns, w, row);
}

int main()
{
    long cases = 0, accepted = 0;
    // ---- the index and parse workspace ----
    const std::vector<unsigned long long> sizes = {0, 1, 13, 14, 15, 16, 17, 255, 256, 16383, 16384, 16385, 32768, 1000003, 80ull << 20,
                                                   (unsigned long long)csvp::MAX_BYTES - 1, (unsigned long long)csvp::MAX_BYTES,
                                                   (unsigned long long)csvp::MAX_BYTES + 1, 1ull << 31, 0xFFFFFFFFull, 1ull << 32,
                                                   1ull << 40, (unsigned long long)SIZE_MAX - 1, (unsigned long long)SIZE_MAX};
    for (unsigned long long n : sizes) {
        ++cases;
        csvp::Plan p = {};
        const bool ok = csvp::plan_of((size_t)n, p);
        const bool valid = n >= 1 && n <= csvp::MAX_BYTES;
        if (ok != valid) { std::printf("%llu bytes: %s\n", n, ok ? "accepted" : "refused"); return 1; }
        if (!ok) continue;
        ++accepted;
        const u128 chunks = ((u128)n + csvp::INDEX_CHUNK - 1) / csvp::INDEX_CHUNK, lines = (u128)n / csvp::MIN_LINE_BYTES + 3;
        const u128 want = up(256) + up(chunks * (csvp::INDEX_CHUNK / 16) * 2) + up(chunks * 4) + up(scan_words(chunks) * 4) + up(lines * 4);
        if ((u128)p.total != want || p.total % 256 || p.n_chunks != (size_t)chunks || p.line_capacity != (size_t)lines ||
            !(p.meta < p.bitmap && p.bitmap < p.counts && p.counts < p.scan_temp && p.scan_temp < p.starts && p.starts < p.total) ||
            p.bitmap - p.meta < 256 || p.counts - p.bitmap < p.n_chunks * (csvp::INDEX_CHUNK / 16) * 2 || p.scan_temp - p.counts < p.n_chunks * 4 ||
            p.total - p.starts < p.line_capacity * 4) {
            std::printf("%llu bytes: total %zu, expected %.0Lf\n", n, p.total, (long double)want);
            return 1;
        }
        // every bit map word the index pass writes and every offset it may hold lie inside their parts
        if (p.n_chunks * (size_t)csvp::INDEX_CHUNK < n || (p.n_chunks - 1) * (size_t)csvp::INDEX_CHUNK >= n || n + 1 > 0xFFFFFFFFull) {
            std::printf("%llu bytes: %zu chunks\n", n, p.n_chunks);
            return 1;
        }
    }
    // ---- the ordering's workspace ----
    const std::vector<long long> rows = {LLONG_MIN, -1, 0, 1, 2047, 2048, 2049, 300000, 1 << 20, csvp::MAX_ROWS, csvp::MAX_ROWS + 1, LLONG_MAX};
    for (long long n : rows) {
        ++cases;
        csvp::OrderPlan p = {};
        const bool ok = csvp::order_plan_of(n, p);
        if (ok != (n >= 1 && n <= csvp::MAX_ROWS)) { std::printf("%lld rows: %s\n", n, ok ? "accepted" : "refused"); return 1; }
        if (!ok) continue;
        ++accepted;
        const u128 cells = 256 * (((u128)n + 2047) / 2048);
        const u128 want = 2 * up((u128)n * 8) + 2 * up((u128)n * 4) + up(((cells + 63) / 64 * 64 + scan_words(cells)) * 4);
        if ((u128)p.total != want || !(p.keys_a < p.keys_b && p.keys_b < p.idx_a && p.idx_a < p.idx_b && p.idx_b < p.temp && p.temp < p.total) ||
            csvp::parse_groups(n) != (unsigned)((n + 255) / 256)) {
            std::printf("%lld rows: total %zu, expected %.0Lf\n", n, p.total, (long double)want);
            return 1;
        }
    }
    // ---- lines in blocks of exactly their size ----
    ysmr_csv::Wanted w7 = {{0, 1, 2, 3, 4, 5, 6}}, w9 = {{1, 2, 3, 4, 5, 6, 7}}, wrev = {{6, 5, 4, 3, 2, 1, 0}};
    struct Line { const char *text; int n_columns; const ysmr_csv::Wanted *w; bool served; };
    const Line lines[] = {
        {"1,2,3.5,4.5,5.5,6.5,7.5", 7, &w7, true}, {"-0.0,5.0,4.0,3.0,2.0,1,0", 7, &wrev, true}, {"7,1,2,3.5,4.5,5.5,6.5,7.5,80.25", 9, &w9, true},
        {",1,2,3.5,4.5,5.5,6.5,7.5,", 9, &w9, true}, {"4294967295,0,1e-300,1E+300,12345678901234567890123.5,0.000001,1", 7, &w7, true},
        {"", 7, &w7, false}, {"1", 7, &w7, false}, {"1,2,3.5,4.5,5.5,6.5,", 7, &w7, false}, {"1,2,3.5,4.5,5.5,6.5,7.", 7, &w7, false},
        {"1,2,3.5,4.5,5.5,6.5,7e", 7, &w7, false}, {"1,2,3.5,4.5,5.5,6.5,7e-", 7, &w7, false}, {"1,2,3.5,4.5,5.5,6.5,-", 7, &w7, false},
        {"1,2,3.5,4.5,5.5,6.5,7.5,", 7, &w7, false}, {"1,2,3.5,4.5,5.5,6.5", 7, &w7, false}, {"4294967296,2,3.5,4.5,5.5,6.5,7.5", 7, &w7, false},
        {"1,2,1e309,4.5,5.5,6.5,7.5", 7, &w7, false}, {"1,2,9e308,4.5,5.5,6.5,7.5", 7, &w7, false}, {",,,,,,", 7, &w7, false},
        {"7,1,2,3.5,4.5,5.5,6.5,7.5", 9, &w9, false}, {"1,2,3.5,4.5,5.5,6.5,99999999999999999999999999999999999999e-99999", 7, &w7, false},
    };
    for (const Line &l : lines) {
        ++cases;
        ysmr_csv::Row row = {};
        if (parse(l.text, l.n_columns, *l.w, row) != l.served) { std::printf("line '%s': %s\n", l.text, l.served ? "not served" : "served"); return 1; }
        accepted += l.served;
    }
    ysmr_csv::Row row = {};
    if (!parse("4294967295,0,1e-300,1E+300,12345678901234567890123.5,0.000001,1", 7, w7, row) || row.id != 4294967295u || row.t != 0u ||
        row.v[0] != 1e-300 || row.v[1] != 1e300 || row.v[3] != 0.000001 || row.v[4] != 1.0) { std::printf("values\n"); return 1; }
    // (a reversed header: the first field is DEGREES_ANGLE, the last TRACK_ID)
    if (!parse("-0.0,5.0,4.0,3.0,2.0,1,0", 7, wrev, row) || row.id != 0u || row.t != 1u || row.v[0] != 2.0 || row.v[3] != 5.0 ||
        row.v[4] != 0.0 || !std::signbit(row.v[4])) { std::printf("values of the reversed line\n"); return 1; }
    std::printf("ok %ld cases, %ld accepted\n", cases, accepted);
    return 0;
}
