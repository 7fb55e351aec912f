"""CPU: the exact heading model (tests/atan2_exact.py) against mpmath -- through the committed fixture everywhere, and
directly where mpmath is installed."""
import math
import os

import numpy as np
import pytest

from atan2_exact import atan2_cr, atan2_scalar, ulp_wiggle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atan2_lattice.npz")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def lattice():
    z = np.load(GOLDEN)
    return z["y"], z["x"], z["atan2"]


def random_pairs(kind, n=100_000):
    """(y, x): magnitudes log-uniform in 1e-300 .. 1e300, mixed signs; 'f32' draws float32-widened mantissas (the exponent
    range is the doubles': the values are what differences and products of float32 columns look like)."""
    rng = np.random.default_rng({"f32": 11, "f64": 12}[kind])
    out = []
    for _ in range(2):
        mant = rng.uniform(1.0, 2.0, n)
        if kind == "f32":
            mant = mant.astype(np.float32).astype(np.float64)
        expo = rng.integers(-996, 997, n)            # 2^-996 .. 2^997 = 1.5e-300 .. 1.3e300
        near = rng.random(n) < 0.5                   # half of the pairs within 2^+-8 of each other: headings off the axes
        out.append((mant, expo, near))
    (my, ey, near), (mx, ex, _) = out
    ey = np.where(near, ex + rng.integers(-8, 9, n), ey).clip(-996, 996)
    y = np.ldexp(my, ey) * rng.choice([-1.0, 1.0], n)
    x = np.ldexp(mx, ex) * rng.choice([-1.0, 1.0], n)
    return y, x


def test_model_matches_the_fixture_bit_for_bit(capsys):
    y, x, want = lattice()
    g = np.arange(-32, 33) * 0.5
    assert len(y) == 65 * 65 and np.array_equal(y.reshape(65, 65)[:, 0], g) and np.array_equal(x.reshape(65, 65)[0], g)
    got = atan2_cr(y, x)
    assert np.array_equal(bits(got), bits(want))
    # not asserted: how far this machine's own libraries are from the model on these arguments (the host spread)
    with np.errstate(all="ignore"):
        off_numpy = int((bits(np.arctan2(y, x)) != bits(got)).sum())
    off_libm = int(sum(math.atan2(b, a) != v or math.copysign(1, math.atan2(b, a)) != math.copysign(1, v)
                       for b, a, v in zip(y.tolist(), x.tolist(), got.tolist())))
    with capsys.disabled():
        print(f"\n[atan2 host spread] of {len(y)} lattice headings: np.arctan2 (NumPy {np.__version__}) differs from the "
              f"correctly rounded value on {off_numpy}, math.atan2 on {off_libm}")


def test_model_exact_cases_and_signs_of_zero():
    pi = math.pi
    cases = [(0.0, 1.5, 0.0), (-0.0, 1.5, -0.0), (0.0, -1.5, pi), (-0.0, -1.5, -pi), (2.0, 0.0, pi / 2), (2.0, -0.0, pi / 2),
             (-2.0, 0.0, -pi / 2), (-2.0, -0.0, -pi / 2), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, pi), (-0.0, -0.0, -pi),
             (math.inf, 1.0, pi / 2), (1.0, -math.inf, pi), (-1.0, math.inf, -0.0)]
    for y, x, want in cases:
        got = atan2_scalar(y, x)
        assert got == want and math.copysign(1, got) == math.copysign(1, want), (y, x, got)
        assert bits(atan2_cr([y], [x]))[0] == bits([want])[0]
    assert math.isnan(atan2_scalar(math.nan, 1.0)) and np.isnan(atan2_cr([1.0, np.nan], [np.nan, np.nan])).all()
    # the smallest results: subnormal, and below half of the smallest subnormal
    assert atan2_scalar(5e-324, 1.0) == 5e-324 and atan2_scalar(-5e-324, 3.0) == -0.0 and atan2_scalar(1e-300, 1e300) == 0.0
    assert atan2_scalar(1e-300, -1e300) == pi and atan2_scalar(1e300, 1e-300) == pi / 2
    assert atan2_cr(np.zeros((0, 3)), 1.0).shape == (0, 3)
    w = ulp_wiggle(np.array([1.0, 1.0, np.nan, -2.0]))
    assert w[0] == np.nextafter(1.0, 2.0) and w[1] == np.nextafter(1.0, 0.0) and np.isnan(w[2]) and w[3] == np.nextafter(-2.0, -3.0)


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_model_matches_mpmath_on_random_pairs(kind):
    mpmath = pytest.importorskip("mpmath")
    from fractions import Fraction
    y, x = random_pairs(kind)
    assert (y > 0).any() and (y < 0).any() and (x > 0).any() and (x < 0).any()
    assert min(np.abs(y).min(), np.abs(x).min()) < 1e-290 and max(np.abs(y).max(), np.abs(x).max()) > 1e290
    got = atan2_cr(y, x)
    assert (got == 0).sum() > 100 and (np.abs(got) < 1e-3).sum() > 10_000            # underflow, and the tiny-heading path
    bad = 0
    with mpmath.workprec(200):
        for b, a, v in zip(y.tolist(), x.tolist(), got.tolist()):
            m = mpmath.atan2(mpmath.mpf(b), mpmath.mpf(a))
            want = float(m)
            if abs(want) < 2.3e-308:                 # subnormal: round the 200-bit value once, not via 53 bits
                sign, man, exp, _ = m._mpf_
                f = Fraction(man) * Fraction(2) ** exp / Fraction(2) ** -1074
                n = f.numerator // f.denominator
                rem = f - n
                n += rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1)
                want = math.ldexp(n, -1074) * (-1.0 if sign else 1.0)
            bad += not (v == want and math.copysign(1, v) == math.copysign(1, want))
    assert bad == 0, f"{bad} of {len(y)} differ from mpmath at 200 bits"


# ---- csrc/atan2_cr.h, run on the host: what k_ev_heading and k_hist compute ------------------------------------------------

def devicelike(y, x):
    from ysmr_amd import _lib
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    out = np.full(len(y), -7.0)
    _lib.check(_lib.lib().ysmr_atan2_devicelike(y.ctypes.data, x.ctypes.data, len(y), out.ctypes.data), "ysmr_atan2_devicelike")
    return out


def test_devicelike_atan2_is_the_model_on_the_lattice_and_the_axes():
    from ysmr_amd import _lib
    assert "ysmr_atan2_devicelike" in _lib.EXPORTS
    y, x, want = lattice()
    assert np.array_equal(bits(devicelike(y, x)), bits(want))
    # every sign-of-zero and axis case, the infinities, NaN; the subnormal results and the tie below an exact quotient
    tiny, inf, nan = 5e-324, np.inf, np.nan
    vals = [0.0, -0.0, 1.5, -1.5, 16.0, -16.0, tiny, -tiny, 3 * tiny, 1e-310, -1e-310, 2.2250738585072014e-308, 1e-300, 1e300,
            -1e300, 1.7976931348623157e308, inf, -inf, 2.0, 3.0, 0.75]
    yy, xx = (a.ravel() for a in np.meshgrid(vals, vals, indexing="ij"))
    got = devicelike(yy, xx)
    ref = atan2_cr(yy, xx)
    assert np.array_equal(bits(got), bits(ref)), [(a, b) for a, b, g, r in zip(yy, xx, got, ref) if bits([g])[0] != bits([r])[0]][:10]
    assert atan2_scalar(3 * tiny, 2.0) == tiny and atan2_scalar(tiny, 2.0) == 0.0      # 1.5 and 0.5 subnormal steps: the value is below
    with_nan = devicelike([nan, 1.0, nan], [1.0, nan, nan])
    assert np.isnan(with_nan).all()
    assert devicelike(np.zeros(0), np.zeros(0)).shape == (0,)


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_devicelike_atan2_is_the_model_on_random_pairs(kind):
    y, x = random_pairs(kind)
    got, want = devicelike(y, x), atan2_cr(y, x)
    off = bits(got) != bits(want)
    assert off.sum() == 0, f"{off.sum()} of {len(y)} differ, first at {(y[off][:3], x[off][:3])}"
    # and the subnormal results in bulk: y / x around 2^-1074 .. 2^-1022
    rng = np.random.default_rng(5)
    ys = np.ldexp(rng.uniform(1, 2, 20_000), rng.integers(-1074, -1000, 20_000)) * rng.choice([-1.0, 1.0], 20_000)
    xs = np.ldexp(rng.uniform(1, 2, 20_000), rng.integers(0, 60, 20_000))
    got, want = devicelike(ys, xs), atan2_cr(ys, xs)
    assert ((np.abs(want) < 2.2e-308) & (want != 0)).sum() > 5000 and np.array_equal(bits(got), bits(want))
