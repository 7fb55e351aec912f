"""The typed device csv reader's arithmetic on the CPU: ``ysmr_csv_parse_typed_devicelike`` (csrc/csv.hip, the text of
csrc/csv_parse.h a line at a time on the host) against the installed ``pandas.read_csv(usecols, dtype)``.  No tolerance: integer
columns compare equal, float columns as uint64 bits (NaN positions and payloads included), dtypes too.  Every kind of text
the reader does not serve is counted, one row at a time, and leaves no value of that row behind."""
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT

NEW_EXPORTS = ("ysmr_csv_parse_typed", "ysmr_csv_parse_typed_devicelike", "ysmr_marks_workspace_bytes", "ysmr_marks_build")
TYPES = {"u": np.uint32, "q": np.int64, "i": np.int32, "b": np.int8, "f": np.float64, "g": np.float64}
FIELDS = [("u", np.uint32), ("q", np.int64), ("i", np.int32), ("b", np.int8), ("f", np.float64), ("g", np.float64, True)]
ROWS = 200_000          # fields per type


def pandas_reads(data, names):
    return pd.read_csv(io.BytesIO(data), sep=",", header=0, usecols=list(names), dtype={k: TYPES[k] for k in names})


def assert_same_bits(columns, ref):
    for name in ref.columns:
        want, got = ref[name].to_numpy(), columns[name]
        assert got.dtype == want.dtype == np.dtype(TYPES[name]), name
        if want.dtype == np.float64:
            got, want = got.view(np.uint64), want.view(np.uint64)
        diff = np.flatnonzero(got != want)
        assert len(diff) == 0, "{}: {} of {} differ, first at row {}: {!r} against pandas' {!r}".format(
            name, len(diff), len(want), diff[0], columns[name][diff[0]], ref[name].to_numpy()[diff[0]])


def served(data, fields=FIELDS):
    from ysmr_amd.helper_file import parse_csv_typed_devicelike
    got = parse_csv_typed_devicelike(data, fields)
    assert got is not None, "the header was refused"
    columns, n, unserved, flags = got
    assert unserved == 0 and flags == 0, (unserved, flags)
    ref = pandas_reads(data, [f[0] for f in fields])
    assert n == len(ref)
    assert_same_bits(columns, ref)
    return columns


def test_the_new_exports_are_declared_and_the_abi_number_stands():
    from ysmr_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b(int|size_t|void)\s+" + name + r"\s*\(", header), name + " is not declared in include/ysmr_hip.h"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert _lib.ABI_VERSION == 15 and L.ysmr_abi_version() == 15
    assert int(re.search(r"#define YSMR_ABI_VERSION\s+(\d+)", header).group(1)) == 15


@pytest.fixture(scope="module")
def big_table():
    rng = np.random.default_rng(20261020)
    n = ROWS
    f = (rng.standard_normal(n) * 10.0 ** rng.integers(-12, 13, n)).astype(np.float64)
    f[::7] = np.round(rng.uniform(0, 4000, len(f[::7])), 3)               # positions as the tracker writes them
    f[::11] = rng.integers(-1000, 1000, len(f[::11])).astype(np.float64)  # "12.0"
    f[5], f[6], f[8] = 0.0, -0.0, 1.7976931348623157e308
    g = f[::-1].copy()
    g[rng.random(n) < 0.1] = np.nan
    u = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    q = rng.integers(-(10 ** 18 - 1), 10 ** 18, n, dtype=np.int64)
    i = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    b = rng.integers(-128, 128, n).astype(np.int8)
    u[:2], q[:2], i[:2], b[:2] = [0, 2 ** 32 - 1], [-(10 ** 18 - 1), 10 ** 18 - 1], [-2 ** 31, 2 ** 31 - 1], [-128, 127]   # the limits
    # ("x0": a column nobody wants)
    df = pd.DataFrame({"u": u, "x0": rng.integers(0, 100, n).astype(np.int64), "q": q, "i": i, "g": g, "b": b, "f": f})
    return df.to_csv(index=False).encode()


def test_two_hundred_thousand_fields_of_every_type_equal_pandas(big_table):
    columns = served(big_table)
    assert len(columns["u"]) == ROWS and np.isnan(columns["g"]).sum() > ROWS // 20
    assert columns["u"][1] == 2 ** 32 - 1 and columns["q"][0] == -(10 ** 18 - 1) and columns["i"][0] == -2 ** 31 and columns["b"][1] == 127


def test_fields_may_be_asked_for_in_any_order_and_number(big_table):
    served(big_table, [("g", np.float64, True), ("u", np.uint32)])
    served(big_table, [("b", np.int8)])
    # the same text under another type: an int8 column read as int64 and as float64
    from ysmr_amd.helper_file import parse_csv_typed_devicelike
    columns, n, unserved, _flags = parse_csv_typed_devicelike(big_table, [("b", np.int64), ("i", np.float64)])
    ref = pd.read_csv(io.BytesIO(big_table), usecols=["b", "i"], dtype={"b": np.int64, "i": np.float64})
    assert unserved == 0 and np.array_equal(columns["b"], ref["b"].to_numpy()) and columns["b"].dtype == np.int64
    assert np.array_equal(columns["i"].view(np.uint64), ref["i"].to_numpy().view(np.uint64))


def test_an_empty_float_field_first_last_and_in_the_middle_is_pandas_nan():
    text = "g,q,f,u,h\n,1,2.5,3,\n4.5,-1,,3,5.0\n,7,,8,\n1.0,2,3.0,4,5.0\n"
    from ysmr_amd.helper_file import parse_csv_typed_devicelike
    fields = [("g", np.float64, True), ("q", np.int64), ("f", np.float64, True), ("u", np.uint32), ("h", np.float64, True)]
    columns, n, unserved, flags = parse_csv_typed_devicelike(text.encode(), fields)
    assert (n, unserved, flags) == (4, 0, 0)
    ref = pd.read_csv(io.StringIO(text), dtype={"g": np.float64, "q": np.int64, "f": np.float64, "u": np.uint32, "h": np.float64})
    for name in ref.columns:
        assert np.array_equal(columns[name].view(np.uint64) if name in "gfh" else columns[name],
                              ref[name].to_numpy().view(np.uint64) if name in "gfh" else ref[name].to_numpy()), name
    assert columns["g"].view(np.uint64)[0] == 0x7FF8000000000000 and columns["h"].view(np.uint64)[2] == 0x7FF8000000000000
    # without the flag an empty float field is not served
    plain = [(f[0], f[1]) for f in fields]
    _c, n, unserved, _f = parse_csv_typed_devicelike(text.encode(), plain)
    assert (n, unserved) == (4, 3)


HEADER = "u,q,i,b,f,g\n"
GOOD = ("1,2,3,4,5.5,6.5", "4294967295,-999999999999999999,-2147483648,-128,-0.0,")
#: a row the reader must not serve, and why
NOT_SERVED = [
    ("4294967296,2,3,4,5.5,6.5", "uint32 + 1"),
    ("-1,2,3,4,5.5,6.5", "a sign on a uint32"),
    ("1,1000000000000000000,3,4,5.5,6.5", "19 digits"),
    ("1,9223372036854775807,3,4,5.5,6.5", "19 digits, int64's largest"),
    ("1,-9223372036854775808,3,4,5.5,6.5", "19 digits, int64's smallest"),
    ("1,2,2147483648,4,5.5,6.5", "int32 + 1"),
    ("1,2,-2147483649,4,5.5,6.5", "int32 - 1"),
    ("1,2,3,128,5.5,6.5", "int8 + 1"),
    ("1,2,3,-129,5.5,6.5", "int8 - 1"),
    (",2,3,4,5.5,6.5", "an empty uint32"),
    ("1,,3,4,5.5,6.5", "an empty int64"),
    ("1,2,,4,5.5,6.5", "an empty int32"),
    ("1,2,3,,5.5,6.5", "an empty int8"),
    ("1,2,3,4,,6.5", "an empty float without the flag"),
    ("1,2,3,-,5.5,6.5", "a sign alone"),
    ("1,2,3,4,nan,6.5", "nan"),
    ("1,2,3,4,5.5,nan", "nan where empty is NaN"),
    ("1,2,3,4,5.5,NA", "NA"),
    ("1,2,3,4,inf,6.5", "inf"),
    ("1,2,3,4,-inf,6.5", "-inf"),
    ("1,2,3,4,+1,6.5", "+1 as a float"),
    ("1,+2,3,4,5.5,6.5", "+2 as an integer"),
    ("1,2,3,4,1.,6.5", "1."),
    ("1,2,3,4, 5.5,6.5", "a blank"),
    ("1,2,3,4,5.5,6.5 ", "a blank at the end"),
    ("1,2,3.0,4,5.5,6.5", "a fraction on an integer"),
    ("1,2,3,4,5.5", "too few fields"),
    ("1,2,3,4,5.5,6.5,7", "too many fields"),
    ("", "an empty line"),
]


def test_eighteen_digits_are_served_and_nineteen_are_not():
    from ysmr_amd.helper_file import parse_csv_typed_devicelike
    text = "q\n999999999999999999\n-999999999999999999\n000000000000000001\n"
    columns = served(text.encode(), [("q", np.int64)])
    assert columns["q"].tolist() == [10 ** 18 - 1, -(10 ** 18 - 1), 1]
    _c, n, unserved, _f = parse_csv_typed_devicelike(b"q\n1000000000000000000\n0000000000000000001\n", [("q", np.int64)])
    assert (n, unserved) == (2, 2)
    # leading zeros in front of a small type's value do not count
    columns = served(b"i,b\n00000000000000000002147483647,-0000000000000000000000128\n", [("i", np.int32), ("b", np.int8)])
    assert columns["i"][0] == 2 ** 31 - 1 and columns["b"][0] == -128


@pytest.mark.parametrize("line,why", NOT_SERVED, ids=[w for _l, w in NOT_SERVED])
def test_a_row_that_is_not_served_is_counted_and_leaves_no_value(line, why):
    from ysmr_amd.helper_file import parse_csv_typed_devicelike
    data = (HEADER + GOOD[0] + "\n" + line + "\n" + GOOD[1] + "\n").encode()
    columns, n, unserved, flags = parse_csv_typed_devicelike(data, FIELDS)
    assert (n, unserved, flags) == (3, 1, 0), why
    ref = pandas_reads((HEADER + GOOD[0] + "\n" + GOOD[1] + "\n").encode(), [f[0] for f in FIELDS])
    for name in ref.columns:
        raw = columns[name].view(np.uint8).reshape(3, -1)
        assert (raw[1] == 0xFF).all(), "{}: a value of the unserved row was written ({})".format(name, why)
        got = columns[name][[0, 2]]
        want = ref[name].to_numpy()
        assert np.array_equal(got.view(np.uint64) if want.dtype == np.float64 else got, want.view(np.uint64) if want.dtype == np.float64 else want), name


def test_headers_and_field_lists_that_are_refused():
    from ysmr_amd import _lib
    from ysmr_amd.helper_file import csv_typed_plan, parse_csv_typed_devicelike
    assert csv_typed_plan(b"a,b,c", ["c", "a"]) == (3, [2, 0])
    assert csv_typed_plan(b"a,b,a", ["a"]) is None and csv_typed_plan(b"a,b", ["c"]) is None
    assert csv_typed_plan("a,b,ä".encode(), ["a"]) is None
    assert csv_typed_plan(",".join(["n%d" % k for k in range(4097)]).encode(), ["n1"]) is None
    assert csv_typed_plan(",".join(["n%d" % k for k in range(4096)]).encode(), ["n4095"]) == (4096, [4095])
    assert parse_csv_typed_devicelike(b"a,b\n1,2\n", [("c", np.int64)]) is None
    with pytest.raises(ValueError):
        parse_csv_typed_devicelike(b"a,b\n1,2\n", [("a", np.float32)])
    with pytest.raises(ValueError):
        parse_csv_typed_devicelike(b"a,b\n1,2\n", [("a", np.int64, True)])
    # the library's own argument checks: a column twice, a column beyond the header, a flag on an integer
    import ctypes
    L = _lib.lib()
    out = np.zeros(4, np.int64)
    n, bad, flags = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_uint32(0)

    def call(n_columns, entries):
        arr = (_lib.CsvField * max(1, len(entries)))()
        for k, (typ, col, flg) in enumerate(entries):
            arr[k].data, arr[k].type, arr[k].column, arr[k].flags = out.ctypes.data, typ, col, flg
        return L.ysmr_csv_parse_typed_devicelike(b"a,b\n1,2\n", 8, n_columns, len(entries), arr, 4, ctypes.byref(n), ctypes.byref(bad), ctypes.byref(flags))

    assert call(2, [(1, 0, 0)]) == _lib.YSMR_OK and out[0] == 1
    for n_columns, entries in ((2, [(1, 0, 0), (1, 0, 0)]), (2, [(1, 2, 0)]), (2, [(1, 0, 1)]), (2, [(5, 0, 0)]), (0, [(1, 0, 0)]),
                               (4097, [(1, 0, 0)]), (2, []), (2, [(4, 0, 2)])):
        assert call(n_columns, entries) == _lib.YSMR_ERR_ARG, (n_columns, entries)
