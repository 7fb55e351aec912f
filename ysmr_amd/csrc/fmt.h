// Text of a float64 as str(numpy.float64) / repr(float) print it, and pandas' reading of that text back -- for the DEVICE
// (round 5: file -> rows; rows.hip has the host form on std::to_chars, which the CPU tests compare this one with).
//   helper_file.py:1403-1478 (save_list: str() of every value), :860-905 (get_data: pandas.read_csv), :1366-1400 (save_df_to_csv)
// Shortest digits that round-trip, by Steele & White / Burger & Dybvig's free-format algorithm in 128-bit fixed point: enough for
// 2^-20 <= |v| < 2^24 (a track's coordinates, sizes and angles; everything else -- and NaN, infinities -- is left to the host:
// `in_range`).  No tables, no division: a digit is at most nine subtractions.  The table writer (table_csv.hip) prints every
// float64: what shortest() declines goes through shortest_wide() further down, the same algorithm on multi-word integers.
#pragma once
#include <stdint.h>
#include "hd.h"
#define YSMR_FMT_HD YSMR_HD_FORCE

namespace ysmr_fmt {

typedef unsigned __int128 u128;

struct Digits {
    char d[20];     // '0' .. '9', the first not '0'
    int n;          // how many (1 .. 17)
    int exp10;      // the value is d[0].d[1]d[2]... x 10^exp10
};

YSMR_FMT_HD uint64_t bits_of(double v) { union { double d; uint64_t u; } c; c.d = v; return c.u; }
YSMR_FMT_HD double double_of(uint64_t u) { union { double d; uint64_t u; } c; c.u = u; return c.d; }

// finite, non-zero, 2^-20 <= |v| < 2^24
YSMR_FMT_HD bool in_range(double v)
{
    const int e = (int)((bits_of(v) >> 52) & 0x7FFu);
    return e >= 1023 - 20 && e < 1023 + 24;
}

// v > 0, in_range(v)
YSMR_FMT_HD void shortest(double v, Digits &out)
{
    const uint64_t b = bits_of(v);
    const uint64_t frac = b & ((1ull << 52) - 1ull);
    const int e2 = (int)((b >> 52) & 0x7FFu) - 1075;        // v = m 2^e2, m = 2^52 + frac
    const uint64_t m = (1ull << 52) | frac;
    constexpr int F = 84;                                    // fixed point: 1.0 = 2^F
    const int sh = e2 + F;                                   // 12 .. 55
    u128 R = (u128)m << sh;
    u128 Mp = (u128)1 << (sh - 1);                           // half the gap to the next double up
    u128 Mm = frac == 0 ? (u128)1 << (sh - 2) : Mp;          // ... down (half as wide below a power of two)
    const bool even = (m & 1ull) == 0;                       // round-to-nearest-even: the boundaries themselves read back as v
    u128 S = (u128)1 << F;
    int k = 0;
    // scale: (R + Mp) / S in [1/10, 1)
    while (even ? R + Mp >= S : R + Mp > S) { S *= 10; ++k; }
    while (!(even ? (R + Mp) * 10 >= S : (R + Mp) * 10 > S)) { R *= 10; Mp *= 10; Mm *= 10; --k; }
    int n = 0;
    while (true) {
        R *= 10; Mp *= 10; Mm *= 10;
        int d = 0;
        while (R >= S) { R -= S; ++d; }
        const bool low = even ? R <= Mm : R < Mm;
        const bool high = even ? R + Mp >= S : R + Mp > S;
        if (!low && !high) { out.d[n++] = (char)('0' + d); continue; }
        if (low && high) {                                   // both neighbours read back as v: the nearer one, a tie to the even digit
            const u128 twice = R * 2;                        // (ties are real: a float32's double has an exact expansion ending in 5)
            d += twice < S ? 0 : (twice > S ? 1 : (d & 1));
        }
        else if (high) d += 1;
        out.d[n++] = (char)('0' + d);
        break;
    }
    out.n = n;
    out.exp10 = k - 1;
}

// CPython's layout of those digits (format_float_short, 'r'): exponent form iff the decimal exponent is < -4 or >= 16,
// otherwise positional with at least ".0".  Returns the end.
YSMR_FMT_HD char *layout(char *p, const Digits &g)
{
    const int nd = g.n, exp10 = g.exp10;
    if (exp10 < -4 || exp10 >= 16) {
        *p++ = g.d[0];
        if (nd > 1) { *p++ = '.'; for (int i = 1; i < nd; ++i) *p++ = g.d[i]; }
        *p++ = 'e';
        *p++ = exp10 < 0 ? '-' : '+';
        int a = exp10 < 0 ? -exp10 : exp10;
        if (a >= 100) { *p++ = (char)('0' + a / 100); a %= 100; }
        *p++ = (char)('0' + a / 10); *p++ = (char)('0' + a % 10);
        return p;
    }
    const int decpt = exp10 + 1;   // digits before the decimal point
    if (decpt <= 0) {
        *p++ = '0'; *p++ = '.';
        for (int i = 0; i < -decpt; ++i) *p++ = '0';
        for (int i = 0; i < nd; ++i) *p++ = g.d[i];
    } else if (decpt >= nd) {
        for (int i = 0; i < nd; ++i) *p++ = g.d[i];
        for (int i = nd; i < decpt; ++i) *p++ = '0';
        *p++ = '.'; *p++ = '0';
    } else {
        for (int i = 0; i < decpt; ++i) *p++ = g.d[i];
        *p++ = '.';
        for (int i = decpt; i < nd; ++i) *p++ = g.d[i];
    }
    return p;
}

// 10^e, 0 <= e <= 44, as pandas' table holds it: the literal 1e<e>, i.e. the correctly rounded double.  10^0 .. 10^22 are
// exact products; the others are spelled out.
YSMR_FMT_HD double pow10_table(int e)
{
    switch (e) {
        case 0: return 1e0; case 1: return 1e1; case 2: return 1e2; case 3: return 1e3; case 4: return 1e4; case 5: return 1e5;
        case 6: return 1e6; case 7: return 1e7; case 8: return 1e8; case 9: return 1e9; case 10: return 1e10; case 11: return 1e11;
        case 12: return 1e12; case 13: return 1e13; case 14: return 1e14; case 15: return 1e15; case 16: return 1e16;
        case 17: return 1e17; case 18: return 1e18; case 19: return 1e19; case 20: return 1e20; case 21: return 1e21;
        case 22: return 1e22; case 23: return 1e23; case 24: return 1e24; case 25: return 1e25; case 26: return 1e26;
        case 27: return 1e27; case 28: return 1e28; case 29: return 1e29; case 30: return 1e30; case 31: return 1e31;
        case 32: return 1e32; case 33: return 1e33; case 34: return 1e34; case 35: return 1e35; case 36: return 1e36;
        case 37: return 1e37; case 38: return 1e38; case 39: return 1e39; case 40: return 1e40; case 41: return 1e41;
        case 42: return 1e42; case 43: return 1e43; default: return 1e44;
    }
}

// pandas' float converter on the text [p, end) of a POSITIVE number laid out by layout() (rows.hip: pandas_parse, the
// restatement of precise_xstrtod in pandas/_libs/src/parser/tokenizer.c): at most 17 digits (leading zeros included) are
// accumulated in a double, the rest only shifts the exponent, and the result is scaled by one multiplication or division with a
// table power of ten.  |exponent| stays below 45 for the numbers shortest() serves.
YSMR_FMT_HD double pandas_parse_positive(const char *p, const char *end)
{
    double number = 0.0;
    int exponent = 0, nd = 0, ndec = 0;
    const int max_digits = 17;
    while (p < end && *p >= '0' && *p <= '9') {
        if (nd < max_digits) { number = number * 10.0 + (double)(*p - '0'); ++nd; }
        else ++exponent;
        ++p;
    }
    if (p < end && *p == '.') {
        ++p;
        while (nd < max_digits && p < end && *p >= '0' && *p <= '9') { number = number * 10.0 + (double)(*p - '0'); ++p; ++nd; ++ndec; }
        if (nd >= max_digits)
            while (p < end && *p >= '0' && *p <= '9') ++p;
        exponent -= ndec;
    }
    if (p < end && (*p == 'e' || *p == 'E')) {
        ++p;
        bool eneg = false;
        if (p < end && *p == '-') { eneg = true; ++p; }
        else if (p < end && *p == '+') ++p;
        int n = 0;
        while (p < end && *p >= '0' && *p <= '9') { n = n * 10 + (*p - '0'); ++p; }
        exponent += eneg ? -n : n;
    }
    if (exponent > 0) number *= pow10_table(exponent);
    else if (exponent < 0) number /= pow10_table(-exponent);
    return number;
}

// One value of a row: its text at p (the end is returned) -- with via_pandas the text of the value pandas reads back from v's
// text, and *v becomes that value.  ok = false: not served here (the caller hands the rows to the host); nothing is written.
YSMR_FMT_HD char *put_value(char *p, double *v, bool via_pandas, bool &ok)
{
    double a = *v;
    const bool neg = (bits_of(a) >> 63) != 0;
    if (neg) a = -a;
    if (a == 0.0) { if (neg) *p++ = '-'; *p++ = '0'; *p++ = '.'; *p++ = '0'; return p; }     // ("-0.0" reads back as -0.0: unchanged)
    if (!in_range(a)) { ok = false; return p; }
    Digits g;
    shortest(a, g);
    char *q = p;
    if (neg) *q++ = '-';
    char *end = layout(q, g);
    if (!via_pandas) return end;
    const double back = pandas_parse_positive(q, end);
    if (back == a) return end;
    if (!in_range(back)) { ok = false; return p; }
    *v = neg ? -back : back;
    shortest(back, g);
    return layout(q, g);
}

YSMR_FMT_HD char *put_u32(char *p, uint32_t v)
{
    char t[10];
    int n = 0;
    do { t[n++] = (char)('0' + v % 10u); v /= 10u; } while (v);
    while (n) *p++ = t[--n];
    return p;
}

// ---- every finite float64: the printer of the rare cell (table_csv.hip: k_table_wide) ---------------------------------------
// The same free-format algorithm as shortest() -- Burger & Dybvig's R, S, M+, M- with the round-to-even boundaries -- on
// integers of WIDE_WORDS x 32 bits instead of 128-bit fixed point, so that it holds for every finite non-zero double, 5e-324
// (2^-1074) to 1.7976931348623157e+308.  The largest numbers met: S = 2^1076 for a subnormal (times ten if the first guess of
// the decimal exponent is one low), 4 x 10^309 < 2^1029 at the top, R + M+ below 10 S in the digit loop: under 2^1084 of the
// 1152 bits.  No tables: a power of ten is multiplied in nine decimal digits at a time.  Slow on purpose (a few thousand word
// operations a value) and not forced inline: it may use scratch memory for its integers, which is why the steady kernels
// never call it.
constexpr int WIDE_WORDS = 36;

struct Wide {
    uint32_t w[WIDE_WORDS];     // little endian; w[n - 1] != 0
    int n;                      // words in use (0: the value is zero)
};

YSMR_HD inline void wide_set(Wide &a, uint64_t m, int shift)        // a = m << shift  (m < 2^54, shift <= 1078)
{
    for (int i = 0; i < WIDE_WORDS; ++i) a.w[i] = 0u;
    const int word = shift >> 5, bit = shift & 31;
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    a.w[word] = lo << bit;
    a.w[word + 1] = (hi << bit) | (bit ? lo >> (32 - bit) : 0u);
    a.w[word + 2] = bit ? hi >> (32 - bit) : 0u;
    a.n = word + 3;
    while (a.n > 0 && a.w[a.n - 1] == 0u) --a.n;
}

YSMR_HD inline void wide_mul_small(Wide &a, uint32_t c)
{
    uint64_t carry = 0;
    for (int i = 0; i < a.n; ++i) {
        const uint64_t t = (uint64_t)a.w[i] * c + carry;
        a.w[i] = (uint32_t)t;
        carry = t >> 32;
    }
    if (carry && a.n < WIDE_WORDS) a.w[a.n++] = (uint32_t)carry;
}

YSMR_HD inline void wide_mul_pow10(Wide &a, int k)
{
    for (; k >= 9; k -= 9) wide_mul_small(a, 1000000000u);
    uint32_t c = 1u;
    for (int i = 0; i < k; ++i) c *= 10u;
    if (c > 1u) wide_mul_small(a, c);
}

YSMR_HD inline int wide_cmp(const Wide &a, const Wide &b)          // -1, 0, 1
{
    if (a.n != b.n) return a.n < b.n ? -1 : 1;
    for (int i = a.n - 1; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}

YSMR_HD inline void wide_add(Wide &out, const Wide &a, const Wide &b)
{
    const int n = a.n > b.n ? a.n : b.n;
    uint64_t carry = 0;
    for (int i = 0; i < n; ++i) {
        const uint64_t t = (uint64_t)(i < a.n ? a.w[i] : 0u) + (i < b.n ? b.w[i] : 0u) + carry;
        out.w[i] = (uint32_t)t;
        carry = t >> 32;
    }
    out.n = n;
    if (carry && out.n < WIDE_WORDS) out.w[out.n++] = (uint32_t)carry;
}

YSMR_HD inline void wide_sub(Wide &a, const Wide &b)               // a -= b, a >= b
{
    uint64_t borrow = 0;
    for (int i = 0; i < a.n; ++i) {
        const uint64_t t = (uint64_t)a.w[i] - (i < b.n ? b.w[i] : 0u) - borrow;
        a.w[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
    while (a.n > 0 && a.w[a.n - 1] == 0u) --a.n;
}

// v > 0 and finite
YSMR_HD inline void shortest_wide(double v, Digits &out)
{
    const uint64_t b = bits_of(v);
    const uint64_t frac = b & ((1ull << 52) - 1ull);
    const int be = (int)((b >> 52) & 0x7FFu);
    const uint64_t m = be ? (1ull << 52) | frac : frac;     // v = m 2^e2
    const int e2 = (be ? be : 1) - 1075;
    const int u = (frac == 0 && be > 1) ? 1 : 0;            // the gap below a power of two is half as wide (not below 2^-1022)
    const bool even = (m & 1ull) == 0;
    Wide R, S, Mp, Mm, T;
    if (e2 >= 0) { wide_set(R, m, e2 + 1 + u); wide_set(S, 1ull, 1 + u); wide_set(Mm, 1ull, e2); wide_set(Mp, 1ull, e2 + u); }
    else { wide_set(R, m, 1 + u); wide_set(S, 1ull, 1 - e2 + u); wide_set(Mm, 1ull, 0); wide_set(Mp, 1ull, u); }
    // a first guess of the decimal exponent from the binary one, floor(e log10 2) + 1; the two loops settle it as in shortest()
    int top = 63;
    while (!((m >> top) & 1ull)) --top;
    int k = (((e2 + top) * 78913) >> 18) + 1;
    if (k > 0) wide_mul_pow10(S, k);
    else if (k < 0) { wide_mul_pow10(R, -k); wide_mul_pow10(Mp, -k); wide_mul_pow10(Mm, -k); }
    // scale: (R + Mp) / S in [1/10, 1)
    for (;;) {
        wide_add(T, R, Mp);
        const int c = wide_cmp(T, S);
        if (!(even ? c >= 0 : c > 0)) break;
        wide_mul_small(S, 10u); ++k;
    }
    for (;;) {
        wide_add(T, R, Mp);
        wide_mul_small(T, 10u);
        const int c = wide_cmp(T, S);
        if (even ? c >= 0 : c > 0) break;
        wide_mul_small(R, 10u); wide_mul_small(Mp, 10u); wide_mul_small(Mm, 10u); --k;
    }
    int n = 0;
    while (true) {
        wide_mul_small(R, 10u); wide_mul_small(Mp, 10u); wide_mul_small(Mm, 10u);
        int d = 0;
        while (wide_cmp(R, S) >= 0) { wide_sub(R, S); ++d; }
        const int cl = wide_cmp(R, Mm);
        const bool low = even ? cl <= 0 : cl < 0;
        wide_add(T, R, Mp);
        const int ch = wide_cmp(T, S);
        const bool high = even ? ch >= 0 : ch > 0;
        if (!low && !high && n < 17) { out.d[n++] = (char)('0' + d); continue; }
        if (low && high) {                                   // the nearer neighbour, a tie to the even digit (as shortest())
            wide_add(T, R, R);
            const int c2 = wide_cmp(T, S);
            d += c2 < 0 ? 0 : (c2 > 0 ? 1 : (d & 1));
        }
        else if (high) d += 1;
        out.d[n++] = (char)('0' + d);
        break;
    }
    out.n = n;
    out.exp10 = k - 1;
}

// ---- a float64 field of a csv as DataFrame.to_csv writes it -----------------------------------------------------------------
// NaN is the empty field, then inf / -inf, 0.0 / -0.0, and every other value its repr.  The widest is 24 bytes
// (-1.2345678901234567e-308).
// a wide cell: finite, non-zero and outside in_range -- the steady row printer copies its text from a side slot
YSMR_FMT_HD bool is_wide_cell(double v)
{
    const uint64_t a = bits_of(v) & 0x7FFFFFFFFFFFFFFFull;
    return a != 0 && a < 0x7FF0000000000000ull && !in_range(double_of(a));
}

// every value that is NOT a wide cell, with shortest(): the steady path.  `g` is the caller's, so that a kernel can keep it
// where dynamic indexing costs no scratch memory (LDS).
YSMR_FMT_HD char *put_f64_steady(char *p, double v, Digits &g)
{
    const uint64_t b = bits_of(v);
    const bool neg = (b >> 63) != 0;
    const uint64_t a = b & 0x7FFFFFFFFFFFFFFFull;
    if (a > 0x7FF0000000000000ull) return p;                 // NaN
    if (neg) *p++ = '-';
    if (a == 0x7FF0000000000000ull) { *p++ = 'i'; *p++ = 'n'; *p++ = 'f'; return p; }
    if (a == 0) { *p++ = '0'; *p++ = '.'; *p++ = '0'; return p; }
    shortest(double_of(a), g);
    return layout(p, g);
}

// a wide cell, with shortest_wide()
YSMR_HD inline char *put_f64_wide(char *p, double v)
{
    const uint64_t b = bits_of(v);
    if (b >> 63) *p++ = '-';
    Digits g;
    shortest_wide(double_of(b & 0x7FFFFFFFFFFFFFFFull), g);
    return layout(p, g);
}

YSMR_HD inline char *put_f64_field(char *p, double v)
{
    if (is_wide_cell(v)) return put_f64_wide(p, v);
    Digits g;
    return put_f64_steady(p, v, g);
}

// Integers straight into their place, last digit first once the count is known: no array of digits that a kernel would have to
// keep in scratch memory (put_u32 above keeps one).
YSMR_FMT_HD char *put_dec32(char *p, uint32_t v)
{
    int n = 1;
    for (uint32_t t = v; t >= 10u; t /= 10u) ++n;
    for (int i = n - 1; i >= 0; --i) { p[i] = (char)('0' + v % 10u); v /= 10u; }
    return p + n;
}

YSMR_FMT_HD char *put_dec64(char *p, uint64_t v)
{
    if (v <= 0xFFFFFFFFull) return put_dec32(p, (uint32_t)v);
    int n = 1;
    for (uint64_t t = v; t >= 10u; t /= 10u) ++n;
    for (int i = n - 1; i >= 0; --i) { p[i] = (char)('0' + (int)(v % 10u)); v /= 10u; }
    return p + n;
}

YSMR_FMT_HD char *put_int64(char *p, int64_t v)
{
    if (v < 0) { *p++ = '-'; return put_dec64(p, 0ull - (uint64_t)v); }    // (-2^63: its own negation as an unsigned number)
    return put_dec64(p, (uint64_t)v);
}

}  // namespace ysmr_fmt
