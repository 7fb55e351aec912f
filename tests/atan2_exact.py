"""The correctly rounded atan2 of doubles, in Python integers: the heading that evaluate_tracks and the angle
histogram are defined by ("The figures").  A double is an exact rational, so atan2(y, x) is worked out in
fixed point with 280 fractional bits behind the result's leading bit and rounded once, to nearest even.  The error
of the fixed-point value is bounded (`_ERR` units in its last place); if the bound straddles a rounding boundary the
model raises instead of guessing -- atan of a non-zero rational is transcendental, so for 280 bits that would need
a run of ~220 zeros or ones behind the 53rd bit.  (One place needs more than bits: a tiny y / x whose quotient is
exactly the middle between two subnormal doubles.  There atan t lies in (t - t^3, t), which is bracketed exactly.)  Needs nothing but the standard library and NumPy;
tests/golden/atan2_lattice.npz pins it against mpmath.

    atan(lo / hi), 0 < lo <= hi:   k = round(256 lo / hi),  atan(lo / hi) = atan(k / 256) + atan(r),
                                   r = (256 lo - k hi) / (256 hi + k lo)  (exact, |r| <= 1 / 512),  atan(r) by its series;
    atan(k / 256) = atan((k - 1) / 256) + atan(256 / (65536 + k (k - 1))),  pi = 4 atan(256 / 256).
"""
import math

import numpy as np

_BITS = 280                  # fractional bits behind the leading bit of the result
_TABLE_BITS = 400
_ERR = 256                   # bound of the error of a value at scale S, in units of 2^-S (see _atan_small)


def _atan_small(num, den, s):
    """atan(num / den) * 2^s for 0 <= num / den <= 1 / 128, as an integer.  Error: under 1 unit from r, and under 3 per
    term (two truncations and what the term before passes on) for at most (s + 14) / 14 terms while s <= 400: under
    100 units."""
    r = (num << s) // den
    r2 = (r * r) >> s
    total = term = r
    k = 1
    while term:
        term = (term * r2) >> s
        k += 2
        total += -(term // k) if k & 2 else term // k
    return total


def _build_table():
    tab = [0]
    for k in range(1, 257):
        tab.append(tab[-1] + _atan_small(256, 65536 + k * (k - 1), _TABLE_BITS))
    return tab                # error under 256 * 100 units of 2^-400: nothing at the scales below (<= 2^-300)


_TABLE = _build_table()


def _rne(a, shift):
    """a / 2^shift rounded to the nearest integer, ties to even (a >= 0, shift >= 1)."""
    fl = a >> shift
    rem = a - (fl << shift)
    half = 1 << (shift - 1)
    if rem > half or (rem == half and fl & 1):
        fl += 1
    return fl


def _to_double(a, s, what, below=None):
    """The double nearest to a value known to lie in [a - _ERR, a + _ERR] / 2^s (or in [below, a] / 2^s), a > 0; raises if
    that does not decide it."""
    e = a.bit_length() - 1 - s                     # a / 2^s in [2^e, 2^(e + 1))
    q = max(e - 52, -1074)                         # the doubles there are multiples of 2^q
    shift = s + q
    assert shift > 64
    lo, hi = (_rne(max(a - _ERR, 0), shift), _rne(a + _ERR, shift)) if below is None else (_rne(below, shift), _rne(a, shift))
    if lo != hi or lo > 1 << 53:
        raise ArithmeticError(f"atan2_cr{what}: {_BITS} bits do not decide the rounding")
    return math.ldexp(lo, q)


def _split(v):
    m, e = math.frexp(v)
    return int(math.ldexp(m, 53)), e - 53          # v = m * 2^e exactly, subnormals included


def _atan2_finite(ay, ax, x_negative):
    """atan2(ay, +-ax) for finite ay, ax > 0."""
    my, ey = _split(ay)
    mx, ex = _split(ax)
    e0 = min(ey, ex)
    p, q = my << (ey - e0), mx << (ex - e0)        # ay / ax = p / q
    swap = p > q
    lo, hi = (q, p) if swap else (p, q)
    gap = hi.bit_length() - lo.bit_length()
    if not swap and not x_negative and gap > 128:
        # t = lo / hi < 2^-127 and t - t^3 / 3 < atan t < t: the t^3 is far behind 280 bits, yet it decides where t itself is
        # the middle between two doubles (which only a subnormal result can be).  Bracket the value instead.
        s = 3 * gap + _BITS
        upper, rem = divmod(lo << s, hi)           # t 2^s, rounded down: t^3 2^s > 2^270 units, so ...
        cube = (upper * upper * upper) >> (2 * s)
        return _to_double(upper - (rem == 0), s, (ay, ax), below=upper - cube)     # ... t - t^3 < atan t <= these
    s = _BITS
    if not swap and not x_negative:                # the result is atan(lo / hi) itself: it may be tiny
        s += max(0, hi.bit_length() - lo.bit_length() + 1)
    k = (512 * lo + hi) // (2 * hi)                # round(256 lo / hi), 0 .. 256
    num, den = 256 * lo - k * hi, 256 * hi + k * lo
    a = _atan_small(abs(num), den, s)
    if k:                                          # (k > 0 means lo / hi >= 1 / 512: s <= _BITS + 10)
        a = (_TABLE[k] >> (_TABLE_BITS - s)) + (a if num >= 0 else -a)
    if swap:
        a = (_TABLE[256] >> (_TABLE_BITS - s - 1)) - a         # pi / 2 - atan(ax / ay)
    if x_negative:
        a = (_TABLE[256] >> (_TABLE_BITS - s - 2)) - a         # pi - ...
    return _to_double(a, s, (ay, -ax if x_negative else ax))


def atan2_scalar(y, x):
    y, x = float(y), float(x)
    if y != y or x != x:
        return math.nan
    if y == 0.0 or x == 0.0 or math.isinf(y) or math.isinf(x):
        # IEEE 754 / C Annex F: +-0 and +-pi on the x axis (the sign of a zero x counts), +-pi/2 on the y axis, multiples
        # of pi/4 at infinity, each constant correctly rounded -- which is what every libm returns
        if y == 0.0:
            return math.copysign(0.0 if math.copysign(1.0, x) > 0 else math.pi, y)
        if x == 0.0:
            return math.copysign(math.pi / 2, y)
        return math.atan2(y, x)
    return math.copysign(_atan2_finite(abs(y), abs(x), x < 0), y)


_CACHE = {}


def atan2_cr(y, x):
    """Correctly rounded ``np.arctan2(y, x)`` for float64 arrays (broadcast against each other); NaN where either is NaN.
    One evaluation per distinct (y, x) pair -- the signs of zeros are distinct -- kept for later calls."""
    y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
    shape = y.shape
    bits = np.stack([np.ascontiguousarray(y).reshape(-1).view(np.uint64), np.ascontiguousarray(x).reshape(-1).view(np.uint64)], axis=1)
    if len(bits) == 0:
        return np.zeros(shape)
    pairs, inverse = np.unique(bits, axis=0, return_inverse=True)
    values = pairs.view(np.float64)
    out = np.empty(len(pairs))
    for j, (key, (yv, xv)) in enumerate(zip(map(tuple, pairs.tolist()), values.tolist())):
        r = _CACHE.get(key)
        if r is None:
            r = atan2_scalar(yv, xv)
            if len(_CACHE) < 1 << 20:
                _CACHE[key] = r
        out[j] = r
    return out[np.asarray(inverse).reshape(-1)].reshape(shape)


def ulp_wiggle(a):
    """`a` with every finite entry moved to the neighbouring double, alternately up and down: what a heading that is
    not correctly rounded may look like.  The tests use it to show that a table can tell the difference."""
    a = np.asarray(a, np.float64)
    up = np.arange(a.size).reshape(a.shape) % 2 == 0
    return np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))


def double_double_constants(n=64):
    """The constants of csrc/atan2_cr.h as (head, tail) pairs of doubles, head + tail the value to ~107 bits: atan(k / n) for
    k = 0 .. n (n divides 256), pi / 2, pi, 1 / 3, 1 / 5, 1 / 7.  `python tests/atan2_exact.py` prints them as C++ hex floats."""
    from fractions import Fraction

    def dd(q):
        head = float(q)                       # (Fraction -> float rounds correctly)
        return head, float(q - Fraction(head))
    scale = Fraction(1, 1 << _TABLE_BITS)
    table = [dd(_TABLE[k * (256 // n)] * scale) for k in range(n + 1)]
    quarter = _TABLE[256] * scale
    return table, {"pi_2": dd(2 * quarter), "pi": dd(4 * quarter), "third": dd(Fraction(1, 3)), "fifth": dd(Fraction(1, 5)),
                   "seventh": dd(Fraction(1, 7))}


if __name__ == "__main__":
    tab, consts = double_double_constants()
    for k, (h, t) in enumerate(tab):
        print(f"    {{{h.hex()}, {t.hex()}}},   // atan({k} / 64)")
    for name, (h, t) in consts.items():
        print(f"{name}: {h.hex()}, {t.hex()}")
