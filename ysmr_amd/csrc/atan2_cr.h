// atan2 of doubles, correctly rounded: the heading of evaluate_tracks (k_ev_heading) and of the angle histogram (k_hist).
// The device library's atan2 is within an ulp, and so is every host's (NumPy's SIMD paths and glibc differ from each other on
// a twelfth of the half-integer pairs): on lattice positions -- raw float32 centres, 'disable gsff' -- a change of heading is
// a whole number of degrees again and again, it is truncated, and an ulp decides.  So the project's heading is the correctly
// rounded one ("The figures"; model: tests/atan2_exact.py), worked out here in double-double (~104 bits):
//     t = lo / hi, lo = min(|y|, |x|), hi = max(|y|, |x|), both scaled by powers of two (exact);
//     k = round(64 t), r = (lo - k/64 hi) / (hi + k/64 lo) (|r| <= 1/128), atan t = atan(k/64) + atan r, atan r by its series
//     (the terms from r^9 on in double: they are below 2^-56 of the sum);
//     |y| > |x|: pi/2 - atan t;  x < 0: pi - that;  the sign of y.
// The double-double result is normalised at the end: its head IS the nearest double unless the value lies within ~2^-100
// (relative) of the middle between two doubles -- atan of a rational is transcendental, no such argument is known, none is among
// the 4225 lattice pairs or the 200 000 random pairs of tests/test_atan2_exact.py.  Results below 2^-1022 (|y| / x tiny, x > 0)
// are rounded once to their subnormal grid.  Zeros, infinities and NaN follow IEEE 754 / C Annex F.
// YSMR_HD: the same code runs on the host (ysmr_atan2_devicelike) for the CPU tests.  No fused multiply-add but the ones written.
#pragma once
#include <cmath>

#include "hd.h"

namespace ysmr {
namespace atan2cr {

struct DD { double h, l; };

// atan(k / 64), pi / 2, pi, 1 / 3, 1 / 5, 1 / 7 as head + tail (python tests/atan2_exact.py prints them)
YSMR_HD_FORCE DD atan_k64(int k)
{
    constexpr double T[65][2] = {
    {0x0.0p+0, 0x0.0p+0},   // atan(0 / 64)
    {0x1.fff555bbb729bp-7, -0x1.220c39d4dff50p-61},   // atan(1 / 64)
    {0x1.ffd55bba97625p-6, -0x1.5ec431444912cp-60},   // atan(2 / 64)
    {0x1.7fb818430da2ap-5, -0x1.86ef8f794f105p-63},   // atan(3 / 64)
    {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60},   // atan(4 / 64)
    {0x1.3f59f0e7c559dp-4, 0x1.ac4ce285df847p-58},   // atan(5 / 64)
    {0x1.7ee182602f10fp-4, -0x1.cfb654c0c3d98p-58},   // atan(6 / 64)
    {0x1.be39ebe6f07c3p-4, 0x1.f7b8f29a05987p-58},   // atan(7 / 64)
    {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59},   // atan(8 / 64)
    {0x1.1e1fafb043727p-3, -0x1.b485914dacf8cp-59},   // atan(9 / 64)
    {0x1.3d6eee8c6626cp-3, 0x1.61a3b0ce9281bp-57},   // atan(10 / 64)
    {0x1.5c9811e3ec26ap-3, -0x1.054ab2c010f3dp-58},   // atan(11 / 64)
    {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58},   // atan(12 / 64)
    {0x1.9a6a8e96c8626p-3, 0x1.cf601e7b4348ep-59},   // atan(13 / 64)
    {0x1.b90d7529260a2p-3, 0x1.17b10d2e0e5abp-61},   // atan(14 / 64)
    {0x1.d77d5df205736p-3, 0x1.c648d1534597ep-57},   // atan(15 / 64)
    {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},   // atan(16 / 64)
    {0x1.09dc597d86362p-2, 0x1.62e47390cb865p-56},   // atan(17 / 64)
    {0x1.18bf5a30bf178p-2, 0x1.30ca4748b1bf9p-57},   // atan(18 / 64)
    {0x1.278372057ef46p-2, -0x1.077cdd36dfc81p-56},   // atan(19 / 64)
    {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57},   // atan(20 / 64)
    {0x1.44aa436c2af0ap-2, -0x1.5d5e43c55b3bap-56},   // atan(21 / 64)
    {0x1.530ad9951cd4ap-2, -0x1.2566480884082p-57},   // atan(22 / 64)
    {0x1.614840309cfe2p-2, -0x1.a725715711f00p-56},   // atan(23 / 64)
    {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56},   // atan(24 / 64)
    {0x1.7d5604b63b3f7p-2, 0x1.69c885c2b249ap-56},   // atan(25 / 64)
    {0x1.8b24d394a1b25p-2, 0x1.b6d0ba3748fa8p-56},   // atan(26 / 64)
    {0x1.98cd5454d6b18p-2, 0x1.9e6c988fd0a77p-56},   // atan(27 / 64)
    {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56},   // atan(28 / 64)
    {0x1.b3a911da65c6cp-2, 0x1.ae187b1ca5040p-56},   // atan(29 / 64)
    {0x1.c0db4c94ec9f0p-2, -0x1.cc1ce70934c34p-56},   // atan(30 / 64)
    {0x1.cde53432c1351p-2, -0x1.a2cfa4418f1adp-56},   // atan(31 / 64)
    {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56},   // atan(32 / 64)
    {0x1.e77eb7f175a34p-2, 0x1.0e53dc1bf3435p-56},   // atan(33 / 64)
    {0x1.f40dd0b541418p-2, -0x1.a3992dc382a23p-57},   // atan(34 / 64)
    {0x1.0039c73c1a40cp-1, -0x1.b32c949c9d593p-55},   // atan(35 / 64)
    {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56},   // atan(36 / 64)
    {0x1.0c6145b5b43dap-1, 0x1.974fa13b5404fp-58},   // atan(37 / 64)
    {0x1.1255d9bfbd2a9p-1, -0x1.2bdaee1c0ee35p-58},   // atan(38 / 64)
    {0x1.1835a88be7c13p-1, 0x1.c621cec00c301p-55},   // atan(39 / 64)
    {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},   // atan(40 / 64)
    {0x1.23b71e2cc9e6ap-1, 0x1.c421c9f38224ep-57},   // atan(41 / 64)
    {0x1.2958e59308e31p-1, -0x1.09e73b0c6c087p-56},   // atan(42 / 64)
    {0x1.2ee628406cbcap-1, 0x1.c5d5e9ff0cf8dp-55},   // atan(43 / 64)
    {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55},   // atan(44 / 64)
    {0x1.39c391cd4171ap-1, -0x1.2304331d8bf46p-55},   // atan(45 / 64)
    {0x1.3f13fb89e96f4p-1, 0x1.ecf8b492644f0p-56},   // atan(46 / 64)
    {0x1.445065b795b56p-1, -0x1.f76d0163f79c8p-56},   // atan(47 / 64)
    {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56},   // atan(48 / 64)
    {0x1.4e8de5bb6ec04p-1, 0x1.4a33dbeb3796cp-55},   // atan(49 / 64)
    {0x1.538f57b89061fp-1, -0x1.1bb74abda520cp-55},   // atan(50 / 64)
    {0x1.587d81f732fbbp-1, -0x1.5e5c9d8c5a950p-56},   // atan(51 / 64)
    {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57},   // atan(52 / 64)
    {0x1.6220d115d7b8ep-1, -0x1.2b785350ee8c1p-57},   // atan(53 / 64)
    {0x1.66d663923e087p-1, -0x1.6ea6febe8bbbap-56},   // atan(54 / 64)
    {0x1.6b798920b3d99p-1, -0x1.a80386188c50ep-55},   // atan(55 / 64)
    {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56},   // atan(56 / 64)
    {0x1.748978fba8e0fp-1, 0x1.7b2a6165884a1p-59},   // atan(57 / 64)
    {0x1.78f6bbd5d315ep-1, 0x1.406a089803740p-55},   // atan(58 / 64)
    {0x1.7d528289fa093p-1, 0x1.560821e2f3aa9p-55},   // atan(59 / 64)
    {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56},   // atan(60 / 64)
    {0x1.85d69576cc2c5p-1, 0x1.6b66e7fc8b8c3p-57},   // atan(61 / 64)
    {0x1.89ff5ff57f1f8p-1, -0x1.55b9a5e177a1bp-55},   // atan(62 / 64)
    {0x1.8e17aa99cc05ep-1, -0x1.ec182ab042f61p-56},   // atan(63 / 64)
    {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55},   // atan(64 / 64)
    };
    return DD{T[k][0], T[k][1]};
}
YSMR_HD_FORCE DD dd_pi_2() { return DD{0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54}; }
YSMR_HD_FORCE DD dd_pi() { return DD{0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53}; }

YSMR_HD_FORCE DD fast_two_sum(double a, double b)          // |a| >= |b| (or a == 0)
{
    const double s = a + b;
    return DD{s, b - (s - a)};
}
YSMR_HD_FORCE DD two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return DD{s, (a - (s - bb)) + (b - bb)};
}
YSMR_HD_FORCE DD two_prod(double a, double b)
{
    const double p = a * b;
    return DD{p, fma(a, b, -p)};
}
YSMR_HD_FORCE DD add(DD a, DD b)                           // accurate sum (error ~2^-105 relative)
{
    DD s = two_sum(a.h, b.h);
    const DD t = two_sum(a.l, b.l);
    s = fast_two_sum(s.h, s.l + t.h);
    return fast_two_sum(s.h, s.l + t.l);
}
YSMR_HD_FORCE DD neg(DD a) { return DD{-a.h, -a.l}; }
YSMR_HD_FORCE DD mul(DD a, DD b)
{
    const DD p = two_prod(a.h, b.h);
    return fast_two_sum(p.h, p.l + (a.h * b.l + a.l * b.h));
}
YSMR_HD_FORCE DD mul_d(DD a, double b)
{
    const DD p = two_prod(a.h, b);
    return fast_two_sum(p.h, p.l + a.l * b);
}
YSMR_HD_FORCE DD div(DD n, DD d)                           // two quotient digits and a third for the tail
{
    const double q1 = n.h / d.h;
    DD r = add(n, neg(mul_d(d, q1)));
    const double q2 = r.h / d.h;
    r = add(r, neg(mul_d(d, q2)));
    const double q3 = r.h / d.h;
    const DD q = fast_two_sum(q1, q2);
    return fast_two_sum(q.h, q.l + q3);
}

// atan(lo / hi) for 0 < lo <= hi, both in [2^-200, 2]
YSMR_HD_FORCE DD atan_ratio(double lo, double hi)
{
    const int k = (int)(lo / hi * 64.0 + 0.5);
    const double c = (double)k * 0.015625;
    // r = (lo - c hi) / (hi + c lo): the products are exact as head + tail
    const DD ch = two_prod(c, hi), cl = two_prod(c, lo);
    const DD num = add(DD{lo, 0.0}, neg(ch)), den = add(DD{hi, 0.0}, cl);
    const DD r = div(num, den);
    const DD z = mul(r, r);
    // atan r = r (1 - z/3 + z^2/5 - z^3/7 + z^4 (1/9 - z/11 + z^2/13 - z^3/15 + z^4/17)),  z <= 2^-14
    const double zh = z.h, z2 = zh * zh;
    const double tail = z2 * z2 * (1.0 / 9.0 + zh * (-1.0 / 11.0 + zh * (1.0 / 13.0 + zh * (-1.0 / 15.0 + zh * (1.0 / 17.0)))));
    DD s = add(mul(z, DD{-0x1.2492492492492p-3, -0x1.2492492492492p-57}), DD{0x1.999999999999ap-3, -0x1.999999999999ap-57});
    s = add(mul(z, s), DD{-0x1.5555555555555p-2, -0x1.5555555555555p-56});
    s = add(mul(z, s), DD{tail, 0.0});
    const DD a = add(r, mul(r, s));                        // r + r (s): the 1 is not rounded into s
    return k ? add(atan_k64(k), a) : a;
}

YSMR_HD_FORCE double atan2_cr(double y, double x)
{
    if (y != y || x != x) return y + x;
    const double ay = fabs(y), ax = fabs(x);
    const bool xneg = __builtin_signbit(x);
    const double inf = HUGE_VAL;
    if (ay == 0.0 || ax == 0.0 || ay == inf || ax == inf) {
        double r;
        if (ay == inf) r = ax == inf ? (xneg ? 0x1.2d97c7f3321d2p+1 : 0x1.921fb54442d18p-1) : 0x1.921fb54442d18p+0;   // 3 pi/4, pi/4, pi/2
        else if (ax == inf || ay == 0.0) r = xneg ? 0x1.921fb54442d18p+1 : 0.0;
        else r = 0x1.921fb54442d18p+0;
        return copysign(r, y);
    }
    const bool swap = ay > ax;
    int e_lo, e_hi;
    const double m_lo = frexp(swap ? ax : ay, &e_lo), m_hi = frexp(swap ? ay : ax, &e_hi);   // mantissas in [0.5, 1)
    const int de = e_lo - e_hi;                            // lo / hi = m_lo / m_hi * 2^de, de <= 1
    if (!swap && !xneg && de < -64) {
        // atan t = t (1 - t^2 / 3 + ...), t < 2^-63: the quotient itself, a hair smaller
        if (de < -1080) return copysign(0.0, y);
        const DD q = div(DD{m_lo, 0.0}, DD{m_hi, 0.0});    // in (0.5, 2)
        int e_q;
        (void)frexp(q.h, &e_q);
        if (de + e_q > -1022) return copysign(ldexp(q.h, de), y);      // normal: scaling is exact
        // subnormal: round q once to multiples of g = 2^(-1074 - de).  big = 2^52 g (q < big): big + q.h rounds to that grid,
        // what it left over and q's tail decide whether the neighbour is nearer.  An exact quotient may sit on a tie: the
        // arc tangent is below it (the -2^-120).
        const double g = ldexp(1.0, -1074 - de), big = ldexp(1.0, -1022 - de), half = 0.5 * g;
        const DD s = fast_two_sum(big, q.h);
        const DD rest = two_sum(s.l, q.l - 0x1p-120);
        double m = s.h;
        if (rest.h > half || (rest.h == half && rest.l > 0.0)) m += g;
        else if (rest.h < -half || (rest.h == -half && rest.l < 0.0)) m -= g;
        return copysign(ldexp(m - big, de), y);
    }
    // (where lo / hi is below 2^-200 the result is pi/2 or pi to far more than 104 bits: any tiny lo will do)
    const DD t = atan_ratio(de < -200 ? ldexp(m_lo, -200) : ldexp(m_lo, de), m_hi);
    DD a = t;
    if (swap) a = add(dd_pi_2(), neg(a));
    if (xneg) a = add(dd_pi(), neg(a));
    return copysign(a.h, y);
}

}  // namespace atan2cr
}  // namespace ysmr
