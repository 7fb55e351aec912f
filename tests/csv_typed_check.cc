// Stand-alone check of the typed csv parse's host-only rules (ysmr_amd/csrc/csv_plan.h: typed_fields_rule) and of its line parser's
// host form (ysmr_amd/csrc/csv_parse.h: parse_line_typed), meant to be built with the host's address and undefined-behaviour
// sanitizers (tests/test_csv_typed_sanitized.py builds and runs it).  Field lists at the limits of their rules; lines that sit in
// heap blocks of exactly their size, so that a fetch beyond a line's end is an error the sanitizer reports, and integers at the
// ends of their types, where a careless accumulation would overflow.  Prints "ok <cases>" and returns 0, or says what failed.
#include "csv_plan.h"
#include "csv_parse.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct HeapText {
    const unsigned char *text;
    int operator()(long long i) const { return text[i]; }
};

static bool parse(const std::string &line, int n_columns, const ysmr_csv::TypedPlan &plan, ysmr_csv::TypedRow &row)
{
    std::vector<unsigned char> block(line.begin(), line.end());      // exactly the line: one byte more is out of bounds
    const HeapText at{block.data()};
    return ysmr_csv::parse_line_typed(at, 0, (long long)block.size(), n_columns, plan, row);
}

// the plan of fields given as (type, column, flags), through the rule, as csv.hip builds it
static bool plan_of(int n_columns, const std::vector<std::vector<int>> &fields, ysmr_csv::TypedPlan &plan)
{
    int32_t type[32], column[32], flags[32];
    int order[32];
    const int n = (int)fields.size();
    if (n > 32) return false;
    for (int k = 0; k < n; ++k) { type[k] = fields[k][0]; column[k] = fields[k][1]; flags[k] = fields[k][2]; }
    if (n > csvp::MAX_FIELDS) return csvp::typed_fields_rule(n_columns, n, type, column, flags, order) == nullptr;   // (refused before `order` is written)
    if (csvp::typed_fields_rule(n_columns, n, type, column, flags, order)) return false;
    plan = ysmr_csv::TypedPlan{};
    plan.n_fields = n;
    for (int k = 0; k < n; ++k) {
        plan.column[k] = column[order[k]];
        plan.type[k] = (uint8_t)type[order[k]];
        plan.flags[k] = (uint8_t)flags[order[k]];
        if (k && plan.column[k] <= plan.column[k - 1]) return false;
    }
    return true;
}

int main()
{
    long cases = 0;
    ysmr_csv::TypedPlan plan;
    // ---- field lists ----
    struct List { int n_columns; std::vector<std::vector<int>> fields; bool ok; };
    std::vector<std::vector<int>> sixteen, seventeen;
    for (int k = 0; k < 17; ++k) { if (k < 16) sixteen.push_back({k % 5, 4095 - 3 * k, 0}); seventeen.push_back({k % 5, k, 0}); }
    const List lists[] = {
        {1, {{0, 0, 0}}, true}, {4096, sixteen, true}, {4096, seventeen, false}, {4097, {{0, 0, 0}}, false}, {0, {{0, 0, 0}}, false},
        {3, {}, false}, {3, {{0, 3, 0}}, false}, {3, {{0, -1, 0}}, false}, {3, {{5, 0, 0}}, false}, {3, {{-1, 0, 0}}, false},
        {3, {{4, 0, 1}}, true}, {3, {{1, 0, 1}}, false}, {3, {{4, 0, 2}}, false}, {3, {{0, 1, 0}, {4, 1, 0}}, false},
        {3, {{0, 2, 0}, {4, 0, 1}, {3, 1, 0}}, true}, {2, {{0, 0, 0}, {0, 1, 0}, {0, 1, 0}}, false},
    };
    for (const List &l : lists) {
        ++cases;
        if (plan_of(l.n_columns, l.fields, plan) != l.ok) { std::printf("field list %ld: %s\n", cases, l.ok ? "refused" : "accepted"); return 1; }
    }
    // ---- lines in blocks of exactly their size: u32, i64, i32, i8, f64, f64 with the empty field as NaN, in columns 0 .. 5 ----
    if (!plan_of(6, {{4, 5, 1}, {0, 0, 0}, {3, 3, 0}, {1, 1, 0}, {4, 4, 0}, {2, 2, 0}}, plan)) { std::printf("the plan of six\n"); return 1; }
    struct Line { const char *text; bool served; };
    const Line lines[] = {
        {"1,2,3,4,5.5,6.5", true}, {"4294967295,-999999999999999999,-2147483648,-128,-0.0,", true}, {"0,999999999999999999,2147483647,127,1e300,", true},
        {"1,2,000000000000000000000000000000000002147483647,-00000000000000000000000000000128,5.5,1e-320", true},
        {"", false}, {"1", false}, {"1,", false}, {"1,2,3,4,5.5", false}, {"1,2,3,4,5.5,6.5,", false}, {"1,2,3,4,,6.5", false}, {",2,3,4,5.5,6.5", false},
        {"1,,3,4,5.5,6.5", false}, {"1,-,3,4,5.5,6.5", false}, {"1,2,3,-", false}, {"1,2,3,4,5.5,-", false}, {"1,2,3,4,5.5,6e", false},
        {"1,1000000000000000000,3,4,5.5,6.5", false}, {"1,9223372036854775807,3,4,5.5,6.5", false}, {"1,-9223372036854775808,3,4,5.5,6.5", false},
        {"1,2,999999999999999999,4,5.5,6.5", false}, {"1,2,3,999999999999999999,5.5,6.5", false}, {"1,2,9999999999999999999,4,5.5,6.5", false},
        {"1,2,2147483648,4,5.5,6.5", false}, {"1,2,-2147483649,4,5.5,6.5", false}, {"1,2,3,128,5.5,6.5", false}, {"1,2,3,-129,5.5,6.5", false},
        {"4294967296,2,3,4,5.5,6.5", false}, {"99999999999,2,3,4,5.5,6.5", false}, {"1,2,3,4,nan,6.5", false}, {"1,2,3,4,5.5,NA", false},
        {"1,2,3,4,inf,6.5", false}, {"1,2,3,4,+1,6.5", false}, {"1,2,3,4,1.,6.5", false}, {"1,2,3,4, 5.5,6.5", false},
    };
    ysmr_csv::TypedRow row;
    for (const Line &l : lines) {
        ++cases;
        std::memset(&row, 0xAB, sizeof(row));
        if (parse(l.text, 6, plan, row) != l.served) { std::printf("line '%s': %s\n", l.text, l.served ? "not served" : "served"); return 1; }
        if (!l.served && row.bits[0] != 0xABABABABABABABABull) { std::printf("line '%s': a value was written\n", l.text); return 1; }
    }
    if (!parse("4294967295,-999999999999999999,-2147483648,-128,-0.0,", 6, plan, row) || row.bits[0] != 4294967295ull ||
        (int64_t)row.bits[1] != -999999999999999999ll || (int32_t)row.bits[2] != INT32_MIN || (int8_t)row.bits[3] != -128 ||
        row.bits[4] != 0x8000000000000000ull || row.bits[5] != ysmr_csv::QUIET_NAN) { std::printf("values\n"); return 1; }
    // ---- 4096 columns, the wanted one last ----
    if (!plan_of(4096, {{1, 4095, 0}}, plan)) { std::printf("the plan of the last column\n"); return 1; }
    std::string wide(4095, ',');
    ++cases;
    if (!parse(wide + "-7", 4096, plan, row) || (int64_t)row.bits[0] != -7 || parse(wide, 4096, plan, row) || parse(wide.substr(1) + "-7", 4096, plan, row)) {
        std::printf("the wide line\n");
        return 1;
    }
    std::printf("ok %ld cases\n", cases);
    return 0;
}
