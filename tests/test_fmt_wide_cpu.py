"""The wide float printer of csrc/fmt.h (``shortest_wide``: Burger & Dybvig on 1152-bit integers) against ``repr(float)``,
through the host export ``ysmr_fmt_f64_text`` -- the text the kernel ``k_table_wide`` compiles.  No GPU.  Every finite non-zero
double must come out as CPython prints it: all powers of two and of ten with their neighbours, the ends of the normal and the
subnormal range, a million random bit patterns; and where the fast printer ``shortest`` applies (2^-20 <= |v| < 2^24) the two
must agree, on a million such values."""
import numpy as np
import pytest

PRINTER_FAST, PRINTER_WIDE, PRINTER_WRITER = 0, 1, 2


def text_of(values, printer):
    """(texts as an 'S24' array, lengths) of ``ysmr_fmt_f64_text``."""
    from ysmr_amd import _lib
    values = np.ascontiguousarray(values, np.float64)
    slots = np.full((len(values), 24), 0xEE, np.uint8)
    lengths = np.zeros(len(values), np.uint8)
    _lib.check(_lib.lib().ysmr_fmt_f64_text(values.ctypes.data, len(values), printer, slots.ctypes.data, lengths.ctypes.data),
               "ysmr_fmt_f64_text")
    return slots.view("S24").ravel(), lengths


def repr_of(values):
    return np.array([repr(v).encode() for v in np.asarray(values, np.float64).tolist()], dtype="S24")


def with_neighbours(values):
    values = np.asarray(values, np.float64)
    both = np.concatenate([values, np.nextafter(values, np.inf), np.nextafter(values, -np.inf)])
    return both[np.isfinite(both) & (both != 0)]


def in_range(values):
    a = np.abs(values)
    return (a >= 2.0 ** -20) & (a < 2.0 ** 24)


def check_against_repr(values):
    values = np.concatenate([values, -values])
    got, lengths = text_of(values, PRINTER_WIDE)
    expect = repr_of(values)
    bad = np.flatnonzero(got != expect)
    assert len(bad) == 0, [(values[i].hex(), got[i], expect[i]) for i in bad[:5]]
    assert np.array_equal(lengths, np.char.str_len(expect))
    return got


def test_powers_of_two_and_their_neighbours():
    check_against_repr(with_neighbours(np.ldexp(1.0, np.arange(-1074, 1024))))


def test_powers_of_ten_and_their_neighbours():
    check_against_repr(with_neighbours(np.array([float("1e{}".format(k)) for k in range(-323, 309)])))


def test_the_ends_of_the_normal_and_the_subnormal_range():
    ends = np.array([5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308])
    got = check_against_repr(with_neighbours(ends))
    assert {b"5e-324", b"2.225073858507201e-308", b"2.2250738585072014e-308", b"1.7976931348623157e+308"} <= set(got.tolist())
    assert text_of([1.5e-13, 5e-324, 1.2345678901234568e17], PRINTER_WIDE)[0].tolist() == [b"1.5e-13", b"5e-324", b"1.2345678901234568e+17"]


def test_a_million_random_bit_patterns():
    rng = np.random.default_rng(20)
    values = rng.integers(0, 2 ** 63, 1_050_000, dtype=np.uint64).view(np.float64)
    values = values[np.isfinite(values) & (values != 0)]
    assert len(values) >= 1_000_000
    check_against_repr(values[:500_000])
    got, _ = text_of(values[500_000:], PRINTER_WIDE)            # (the other half with its sign as drawn: positive)
    assert np.array_equal(got, repr_of(values[500_000:]))


def test_the_two_printers_agree_on_a_million_values_in_range():
    rng = np.random.default_rng(21)
    values = np.ldexp(rng.uniform(1.0, 2.0, 1_000_000), rng.integers(-20, 24, 1_000_000)) * rng.choice([-1.0, 1.0], 1_000_000)
    few = rng.random(len(values)) < 0.3                          # values of few digits: float32 widened, as a table's sizes are
    values[few] = np.float32(values[few]).astype(np.float64)
    values = values[in_range(values)]
    assert len(values) > 990_000
    fast, fast_len = text_of(values, PRINTER_FAST)
    wide, wide_len = text_of(values, PRINTER_WIDE)
    expect = repr_of(values)
    assert np.array_equal(fast, expect) and np.array_equal(wide, expect)
    assert np.array_equal(fast_len, wide_len)
    assert np.array_equal(text_of(values, PRINTER_WRITER)[0], expect)


def test_what_the_fast_printer_declines_and_what_the_writer_prints_for_the_rest():
    wide_cells = np.array([1e-14, -3e-7, 2.0 ** -20 * (1 - 2.0 ** -53), 2.0 ** 24, 1e300, 5e-324])
    assert text_of(wide_cells, PRINTER_FAST)[1].tolist() == [255] * len(wide_cells)
    assert np.array_equal(text_of(wide_cells, PRINTER_WRITER)[0], repr_of(wide_cells))
    special = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf])
    for printer in (PRINTER_FAST, PRINTER_WIDE, PRINTER_WRITER):
        got, lengths = text_of(special, printer)
        assert got.tolist() == [b"0.0", b"-0.0", b"", b"", b"inf", b"-inf"]          # DataFrame.to_csv's fields
        assert lengths.tolist() == [3, 4, 0, 0, 3, 4]


def test_argument_checks():
    from ysmr_amd import _lib
    L = _lib.lib()
    one = np.ones(1)
    out, n = np.zeros(24, np.uint8), np.zeros(1, np.uint8)
    assert L.ysmr_fmt_f64_text(one.ctypes.data, 1, 3, out.ctypes.data, n.ctypes.data) == _lib.YSMR_ERR_ARG
    assert L.ysmr_fmt_f64_text(None, 1, 1, out.ctypes.data, n.ctypes.data) == _lib.YSMR_ERR_ARG
    assert L.ysmr_fmt_f64_text(one.ctypes.data, -1, 1, out.ctypes.data, n.ctypes.data) == _lib.YSMR_ERR_ARG
    assert L.ysmr_fmt_f64_text(None, 0, 1, None, None) == _lib.YSMR_OK
