// The text of a track table read back: one line of a `*_list.csv` / `*_selected_data.csv` -> the seven values pandas.read_csv
// gives for it under upstream's default dtype and usecols (helper_file.py:881-889), for the DEVICE and the host alike
// (csv.hip: k_csv_parse and ysmr_csv_parse_devicelike share this text; fmt.h is the inverse direction).
//
// Served, and nothing else:
//   * a line of exactly n_columns comma-separated fields; the seven wanted ones stand at the positions the host found in the
//     header, every other field is skipped whatever bytes it holds (the index pass has refused '"', '\r', NUL and bytes >= 0x80
//     for the whole file);
//   * TRACK_ID, POSITION_T: 1 .. 10 decimal digits, value <= 2^32 - 1 (leading zeros allowed);
//   * the five float columns: -?digits(.digits)?([eE][+-]?digits)? with 1 .. 4 exponent digits, read the way pandas'
//     precise_xstrtod reads it (pandas/_libs/src/parser/tokenizer.c; rows.hip: pandas_parse): the first 17 digits -- leading
//     zeros included -- accumulated in a double, later integer digits shift the exponent, later fraction digits are dropped,
//     then ONE multiplication or division by a table power of ten (two divisions below 1e-308, as pandas does).  The table
//     holds the correctly rounded literals 1e0 .. 1e308; a final decimal exponent outside POW10_MIN .. POW10_MAX, or a result
//     that is not finite, is not served.  repr(float) of a double in 1e-300 .. 1e300 ends between -316 and +300.
// Everything else -- an empty field, nan / inf, a leading '+' or blank, "1." or ".5", '_', a fraction or a sign on an integer,
// too few or too many fields, an empty line -- returns false: the row is counted unserved, no value of it is written and the
// caller reads the whole file with pandas.
#pragma once
#include <stdint.h>
#include "hd.h"
#ifndef YSMR_FMT_HD
#define YSMR_FMT_HD YSMR_HD_FORCE
#endif

namespace ysmr_csv {

constexpr int WANTED = 7;               // TRACK_ID, POSITION_T, POSITION_X, POSITION_Y, WIDTH, HEIGHT, DEGREES_ANGLE
constexpr int POW10_MAX = 308;          // final decimal exponents served
constexpr int POW10_MIN = -325;
constexpr int MAX_COLUMNS = 4096;

// flags of a file (ysmr_csv_index; any of them: not served)
constexpr uint32_t FLAG_QUOTE = 1u, FLAG_CR = 2u, FLAG_NOT_PLAIN = 4u, FLAG_TOO_MANY_LINES = 8u;

struct Row { uint32_t id, t; double v[5]; };

// 10^e, 0 <= e <= 308, as pandas' table holds it: the literal 1e<e>, i.e. the correctly rounded double
YSMR_FMT_HD double pow10_table(int e)
{
    static const double p[] = {
        1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21,
        1e22, 1e23, 1e24, 1e25, 1e26, 1e27, 1e28, 1e29, 1e30, 1e31, 1e32, 1e33, 1e34, 1e35, 1e36, 1e37, 1e38, 1e39, 1e40, 1e41,
        1e42, 1e43, 1e44, 1e45, 1e46, 1e47, 1e48, 1e49, 1e50, 1e51, 1e52, 1e53, 1e54, 1e55, 1e56, 1e57, 1e58, 1e59, 1e60, 1e61,
        1e62, 1e63, 1e64, 1e65, 1e66, 1e67, 1e68, 1e69, 1e70, 1e71, 1e72, 1e73, 1e74, 1e75, 1e76, 1e77, 1e78, 1e79, 1e80, 1e81,
        1e82, 1e83, 1e84, 1e85, 1e86, 1e87, 1e88, 1e89, 1e90, 1e91, 1e92, 1e93, 1e94, 1e95, 1e96, 1e97, 1e98, 1e99, 1e100, 1e101,
        1e102, 1e103, 1e104, 1e105, 1e106, 1e107, 1e108, 1e109, 1e110, 1e111, 1e112, 1e113, 1e114, 1e115, 1e116, 1e117, 1e118,
        1e119, 1e120, 1e121, 1e122, 1e123, 1e124, 1e125, 1e126, 1e127, 1e128, 1e129, 1e130, 1e131, 1e132, 1e133, 1e134, 1e135,
        1e136, 1e137, 1e138, 1e139, 1e140, 1e141, 1e142, 1e143, 1e144, 1e145, 1e146, 1e147, 1e148, 1e149, 1e150, 1e151, 1e152,
        1e153, 1e154, 1e155, 1e156, 1e157, 1e158, 1e159, 1e160, 1e161, 1e162, 1e163, 1e164, 1e165, 1e166, 1e167, 1e168, 1e169,
        1e170, 1e171, 1e172, 1e173, 1e174, 1e175, 1e176, 1e177, 1e178, 1e179, 1e180, 1e181, 1e182, 1e183, 1e184, 1e185, 1e186,
        1e187, 1e188, 1e189, 1e190, 1e191, 1e192, 1e193, 1e194, 1e195, 1e196, 1e197, 1e198, 1e199, 1e200, 1e201, 1e202, 1e203,
        1e204, 1e205, 1e206, 1e207, 1e208, 1e209, 1e210, 1e211, 1e212, 1e213, 1e214, 1e215, 1e216, 1e217, 1e218, 1e219, 1e220,
        1e221, 1e222, 1e223, 1e224, 1e225, 1e226, 1e227, 1e228, 1e229, 1e230, 1e231, 1e232, 1e233, 1e234, 1e235, 1e236, 1e237,
        1e238, 1e239, 1e240, 1e241, 1e242, 1e243, 1e244, 1e245, 1e246, 1e247, 1e248, 1e249, 1e250, 1e251, 1e252, 1e253, 1e254,
        1e255, 1e256, 1e257, 1e258, 1e259, 1e260, 1e261, 1e262, 1e263, 1e264, 1e265, 1e266, 1e267, 1e268, 1e269, 1e270, 1e271,
        1e272, 1e273, 1e274, 1e275, 1e276, 1e277, 1e278, 1e279, 1e280, 1e281, 1e282, 1e283, 1e284, 1e285, 1e286, 1e287, 1e288,
        1e289, 1e290, 1e291, 1e292, 1e293, 1e294, 1e295, 1e296, 1e297, 1e298, 1e299, 1e300, 1e301, 1e302, 1e303, 1e304, 1e305,
        1e306, 1e307, 1e308};
    static_assert(sizeof(p) / sizeof(p[0]) == POW10_MAX + 1, "1e0 .. 1e308");
    return p[e];
}

YSMR_FMT_HD bool is_digit(int c) { return c >= '0' && c <= '9'; }

// A wanted integer field at [p, end) of the text `at` fetches (at(i): byte i, 0 <= i < end).  Returns the position behind the
// field -- end, or that of its ',' -- or -1: not served.
template <class Fetch>
YSMR_FMT_HD long long parse_u32(const Fetch &at, long long p, long long end, uint32_t &out)
{
    uint64_t v = 0;
    int nd = 0;
    while (p < end) {
        const int c = at(p);
        if (!is_digit(c)) break;
        if (++nd > 10) return -1;
        v = v * 10u + (uint64_t)(c - '0');
        ++p;
    }
    if (nd == 0 || v > 0xFFFFFFFFull) return -1;
    if (p < end && at(p) != ',') return -1;
    out = (uint32_t)v;
    return p;
}

// A wanted float field, as pandas' precise_xstrtod reads it (see the head of this file).
template <class Fetch>
YSMR_FMT_HD long long parse_f64(const Fetch &at, long long p, long long end, double &out)
{
    bool neg = false;
    if (p < end && at(p) == '-') { neg = true; ++p; }
    double number = 0.0;
    long long exponent = 0;
    int nd = 0, ndec = 0;
    const int max_digits = 17;
    int c = p < end ? at(p) : ',';
    if (!is_digit(c)) return -1;                                  // (empty, '+', blank, '.', nan, inf)
    while (is_digit(c)) {
        if (nd < max_digits) { number = number * 10.0 + (double)(c - '0'); ++nd; }
        else ++exponent;
        ++p;
        c = p < end ? at(p) : ',';
    }
    if (c == '.') {
        ++p;
        c = p < end ? at(p) : ',';
        if (!is_digit(c)) return -1;                              // ("1.": pandas reads it, this grammar does not)
        while (is_digit(c)) {
            if (nd < max_digits) { number = number * 10.0 + (double)(c - '0'); ++nd; ++ndec; }
            ++p;
            c = p < end ? at(p) : ',';
        }
        exponent -= ndec;
    }
    if (neg) number = -number;
    if (c == 'e' || c == 'E') {
        ++p;
        c = p < end ? at(p) : ',';
        bool eneg = false;
        if (c == '-' || c == '+') { eneg = c == '-'; ++p; c = p < end ? at(p) : ','; }
        int n = 0, ne = 0;
        while (is_digit(c)) {
            if (++ne > 4) return -1;
            n = n * 10 + (c - '0');
            ++p;
            c = p < end ? at(p) : ',';
        }
        if (ne == 0) return -1;
        exponent += eneg ? -n : n;
    }
    if (c != ',') return -1;
    if (exponent > POW10_MAX || exponent < POW10_MIN) return -1;
    if (exponent > 0) number *= pow10_table((int)exponent);
    else if (exponent < -308) { number /= pow10_table((int)(-308 - exponent)); number /= pow10_table(308); }
    else number /= pow10_table((int)-exponent);
    // (an overflow is an error to pandas, not a value)
    union { double d; uint64_t u; } bits;
    bits.d = number;
    if (((bits.u >> 52) & 0x7FFu) == 0x7FFu) return -1;
    out = number;
    return p;
}

struct Wanted { int32_t column[WANTED]; };      // the position of each wanted name in the header, all distinct, < n_columns

// The line [begin, end) (without its '\n').  true: served, `row` holds its seven values.
template <class Fetch>
YSMR_FMT_HD bool parse_line(const Fetch &at, long long begin, long long end, int n_columns, const Wanted &w, Row &row)
{
    if (end <= begin) return false;                               // an empty line
    long long p = begin;
    uint32_t id = 0, t = 0;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    for (int col = 0; col < n_columns; ++col) {
        if (col) {
            if (p >= end) return false;                           // too few fields
            ++p;                                                  // (the ',' the field before stopped at)
        }
        int slot = -1;
#pragma unroll
        for (int k = 0; k < WANTED; ++k) slot = w.column[k] == col ? k : slot;
        if (slot < 0) {
            while (p < end && at(p) != ',') ++p;
        } else if (slot < 2) {
            uint32_t u = 0;
            p = parse_u32(at, p, end, u);
            if (p < 0) return false;
            if (slot == 0) id = u; else t = u;
        } else {
            double d = 0.0;
            p = parse_f64(at, p, end, d);
            if (p < 0) return false;
            v0 = slot == 2 ? d : v0; v1 = slot == 3 ? d : v1; v2 = slot == 4 ? d : v2; v3 = slot == 5 ? d : v3; v4 = slot == 6 ? d : v4;
        }
    }
    if (p != end) return false;                                   // too many fields
    row.id = id; row.t = t;
    row.v[0] = v0; row.v[1] = v1; row.v[2] = v2; row.v[3] = v3; row.v[4] = v4;
    return true;
}

// ---- the typed parse: 1 .. 16 wanted columns of the table writer's five types (ysmr_csv_parse_typed, csv.hip) ----------------
// What pandas.read_csv(usecols, dtype) gives for a line, for the dtypes uint32 / int64 / int32 / int8 / float64:
//   * U32: parse_u32 above;
//   * I64: -?digits, 1 .. 18 digits in all; I32, I8: -?digits with at most 18 digits behind the leading zeros, the value
//     inside the type;
//   * F64: parse_f64 above; with TYPED_EMPTY_IS_NAN an empty field is served too and is the quiet NaN pandas gives it.
// Everything else (see the head of this file; an empty integer field, a value out of range) is not served.
constexpr int MAX_FIELDS = 16;
constexpr int TYPE_U32 = 0, TYPE_I64 = 1, TYPE_I32 = 2, TYPE_I8 = 3, TYPE_F64 = 4;      // YSMR_COL_* of include/ysmr_hip.h
constexpr int TYPED_EMPTY_IS_NAN = 1;                                                  // YSMR_CSV_EMPTY_IS_NAN
constexpr uint64_t QUIET_NAN = 0x7FF8000000000000ull;

// the wanted fields in the order of their columns: all lanes of a wave look at column `col` in the same iteration, so
// "is this column wanted, and as what" is one compare with the next wanted position, the same for every lane
struct TypedPlan {
    int32_t n_fields;
    int32_t column[MAX_FIELDS];         // ascending
    uint8_t type[MAX_FIELDS], flags[MAX_FIELDS];
};
struct TypedRow { uint64_t bits[MAX_FIELDS]; };     // field k's value in the low bytes of bits[k], in the order of the plan

// -?digits at [p, end): at most max_digits digits (behind the leading zeros if zeros_free), lo <= value <= hi
template <class Fetch>
YSMR_FMT_HD long long parse_int(const Fetch &at, long long p, long long end, int max_digits, bool zeros_free, int64_t lo, int64_t hi,
                                int64_t &out)
{
    bool neg = false;
    if (p < end && at(p) == '-') { neg = true; ++p; }
    int64_t v = 0;
    int nd = 0, any = 0;
    while (p < end) {
        const int c = at(p);
        if (!is_digit(c)) break;
        any = 1;
        if (!(zeros_free && nd == 0 && c == '0') && ++nd > max_digits) return -1;
        v = v * 10 + (int64_t)(c - '0');             // (18 digits: below 2^63)
        ++p;
    }
    if (!any) return -1;
    if (p < end && at(p) != ',') return -1;
    if (neg) v = -v;
    if (v < lo || v > hi) return -1;
    out = v;
    return p;
}

// The line [begin, end) (without its '\n').  true: served, row.bits[k] holds field k for every k < plan.n_fields.
template <class Fetch>
YSMR_FMT_HD bool parse_line_typed(const Fetch &at, long long begin, long long end, int n_columns, const TypedPlan &plan, TypedRow &row)
{
    if (end <= begin) return false;                               // an empty line
    long long p = begin;
    uint64_t v[MAX_FIELDS];
#pragma unroll
    for (int k = 0; k < MAX_FIELDS; ++k) v[k] = 0;
    int next = 0, want = plan.column[0];
    for (int col = 0; col < n_columns; ++col) {
        if (col) {
            if (p >= end) return false;                           // too few fields
            ++p;                                                  // (the ',' the field before stopped at)
        }
        if (col != want) {
            while (p < end && at(p) != ',') ++p;
            continue;
        }
        const int type = plan.type[next];
        uint64_t bits = 0;
        if (type == TYPE_F64) {
            if ((plan.flags[next] & TYPED_EMPTY_IS_NAN) && (p >= end || at(p) == ',')) bits = QUIET_NAN;
            else {
                union { double d; uint64_t u; } u;
                u.d = 0.0;
                p = parse_f64(at, p, end, u.d);
                bits = u.u;
            }
        } else if (type == TYPE_U32) {
            uint32_t u = 0;
            p = parse_u32(at, p, end, u);
            bits = u;
        } else {
            int64_t i = 0;
            if (type == TYPE_I64) p = parse_int(at, p, end, 18, false, INT64_MIN, INT64_MAX, i);
            else if (type == TYPE_I32) p = parse_int(at, p, end, 18, true, INT32_MIN, INT32_MAX, i);
            else p = parse_int(at, p, end, 18, true, INT8_MIN, INT8_MAX, i);
            bits = (uint64_t)i;
        }
        if (p < 0) return false;
        // (no indexing by `next`: on the device the values stay in registers)
#pragma unroll
        for (int k = 0; k < MAX_FIELDS; ++k) v[k] = next == k ? bits : v[k];
        ++next;
        want = next < plan.n_fields ? plan.column[next] : -1;
    }
    if (p != end) return false;                                   // too many fields
#pragma unroll
    for (int k = 0; k < MAX_FIELDS; ++k) row.bits[k] = v[k];
    return true;
}

// field k of a served row into its column
YSMR_FMT_HD void store_typed(void *data, int type, long long r, uint64_t bits)
{
    if (type == TYPE_F64 || type == TYPE_I64) ((uint64_t *)data)[r] = bits;
    else if (type == TYPE_I8) ((int8_t *)data)[r] = (int8_t)bits;
    else ((uint32_t *)data)[r] = (uint32_t)bits;
}

// ---- the kinds of a file's columns: what pandas.read_csv would infer, as far as the typed parse can serve it -----------------
// (ysmr_csv_column_kinds, csv.hip.)  Three bits per column, ORed over the lines:
//   KIND_NOT_INT     a field that is not -?[0-9]{1,18} (what parse_int reads for TYPE_I64)
//   KIND_NOT_NUMBER  a field that is neither empty nor a float64 field parse_f64 serves -- and a run of more than 18 digits
//                    with no '.' or exponent: pandas makes such a column int64, uint64 or object, none of which is guessed at
//   KIND_EMPTY       an empty field
// and one bit for the file: KIND_BAD_LINE, a line that is empty (pandas skips it) or whose field count is not n_columns.
// No bit: the column is int64.  Only NOT_INT / EMPTY: it is float64, NaN where a field is empty.
constexpr uint32_t KIND_NOT_INT = 1u, KIND_NOT_NUMBER = 2u, KIND_EMPTY = 4u, KIND_BAD_LINE = 1u;
constexpr int KIND_WORDS = MAX_FIELDS + 1;          // a word per column, then the file's

// the field at [p, end): its bits into `bits`; returns the position behind it -- end, or that of its ','
template <class Fetch>
YSMR_FMT_HD long long classify_field(const Fetch &at, long long p, long long end, uint32_t &bits)
{
    if (p >= end || at(p) == ',') { bits = KIND_EMPTY | KIND_NOT_INT; return p; }
    int64_t i = 0;
    long long q = parse_int(at, p, end, 18, false, INT64_MIN, INT64_MAX, i);
    if (q >= 0) { bits = 0u; return q; }
    q = p + (at(p) == '-' ? 1 : 0);
    const long long digits_from = q;
    while (q < end && is_digit(at(q))) ++q;
    if (q > digits_from && (q >= end || at(q) == ',')) { bits = KIND_NOT_INT | KIND_NOT_NUMBER; return q; }    // (more than 18 digits)
    double d = 0.0;
    q = parse_f64(at, p, end, d);
    if (q >= 0) { bits = KIND_NOT_INT; return q; }
    bits = KIND_NOT_INT | KIND_NOT_NUMBER;
    q = p;
    while (q < end && at(q) != ',') ++q;
    return q;
}

}  // namespace ysmr_csv
