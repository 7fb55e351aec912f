"""The device csv reader's arithmetic on the CPU: ``ysmr_csv_parse_devicelike`` (csrc/csv.hip, the text of csrc/csv_parse.h a
line at a time on the host) against the installed ``pandas.read_csv`` with upstream's dtype and usecols.  No tolerance: the
integer columns compare equal, the float columns as uint64 bits (so -0.0 and the last bit count), dtypes too.  Every kind
of text the reader does not serve is counted, one at a time, and leaves no value behind."""
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest

import select_tables as st
from conftest import ROOT

NAMES = ["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE"]
HEADER = ",".join(NAMES) + "\n"
NEW_EXPORTS = ("ysmr_csv_workspace_bytes", "ysmr_csv_index", "ysmr_csv_parse", "ysmr_csv_order_workspace_bytes", "ysmr_csv_order",
               "ysmr_csv_geometry", "ysmr_csv_parse_devicelike")


def pandas_reads(data):
    from ysmr_amd.helper_file import _DTYPES
    return pd.read_csv(io.BytesIO(data), sep=",", header=0, usecols=list(_DTYPES), dtype=_DTYPES)


def assert_same_bits(columns, positions, ref):
    """`columns` (in the order of NAMES) against the DataFrame pandas read."""
    assert list(ref.columns) == [NAMES[k] for k in sorted(range(7), key=lambda k: positions[k])]
    for k, name in enumerate(NAMES):
        want = ref[name].to_numpy()
        assert columns[k].dtype == want.dtype == (np.uint32 if k < 2 else np.float64), name
        if k < 2:
            assert np.array_equal(columns[k], want), name
        else:
            diff = np.flatnonzero(columns[k].view(np.uint64) != want.view(np.uint64))
            assert len(diff) == 0, "{}: {} of {} differ, first at row {}: {!r} against pandas' {!r}".format(
                name, len(diff), len(want), diff[0], columns[k][diff[0]], want[diff[0]])


def served(data):
    from ysmr_amd.helper_file import parse_csv_devicelike
    got = parse_csv_devicelike(data)
    assert got is not None, "the header was refused"
    columns, n, unserved, flags, positions = got
    assert unserved == 0 and flags == 0, (unserved, flags)
    ref = pandas_reads(data)
    assert n == len(ref)
    assert_same_bits(columns, positions, ref)
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


def test_geometry_and_workspace_sizes():
    from ysmr_amd import _lib
    L = _lib.lib()
    chunk, rows, span = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    L.ysmr_csv_geometry(ctypes.byref(chunk), ctypes.byref(rows), ctypes.byref(span))
    assert chunk.value > 0 and chunk.value % 16 == 0 and rows.value > 0 and rows.value % 64 == 0 and span.value % 16 == 0
    assert span.value >= 100 * rows.value          # the lines of a list are about 100 bytes
    assert L.ysmr_csv_workspace_bytes(0) == 0
    assert L.ysmr_csv_workspace_bytes(2 ** 31) == 0 and L.ysmr_csv_workspace_bytes(2 ** 64 - 1) == 0
    small, large = L.ysmr_csv_workspace_bytes(1), L.ysmr_csv_workspace_bytes(80 << 20)
    assert 0 < small < large < 2 * (80 << 20)
    assert L.ysmr_csv_order_workspace_bytes(0) == 0 and L.ysmr_csv_order_workspace_bytes(2 ** 31) == 0
    assert L.ysmr_csv_order_workspace_bytes(1000) >= 24 * 1000


def test_a_tracker_table_from_the_projects_formatter():
    from ysmr_amd.helper_file import rows_to_csv_bytes
    rows = st.value_mix_rows(40000)
    for via_pandas in (True, False):
        data = rows_to_csv_bytes(rows, via_pandas=via_pandas)
        columns = served(data)
        assert np.array_equal(columns[0], rows["track_id"].astype(np.uint32))
    served(rows_to_csv_bytes(rows[:1]))
    served(rows_to_csv_bytes(rows[:3])[:-1])           # no final newline


def field_texts(seed, n):
    """Float field texts of many kinds, `n` of each."""
    rng = np.random.default_rng(seed)
    out = []
    bits = rng.integers(0, 2 ** 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    doubles = bits.view(np.float64)
    doubles = doubles[np.isfinite(doubles) & (np.abs(doubles) >= 1e-300) & (np.abs(doubles) <= 1e300)]
    out += [repr(float(v)) for v in doubles]                                          # every magnitude of 1e-300 .. 1e300
    out += [repr(float(v)) for v in rng.uniform(-2000, 2000, n)]
    out += [repr(float(np.float32(v))) for v in rng.uniform(-90, 4000, n)]
    out += [repr(float(v)) for v in 10.0 ** rng.uniform(-30, 30, n) * rng.choice([-1, 1], n)]
    digits = lambda k: "".join(rng.choice(list("0123456789"), k))                     # noqa: E731
    for nd in (16, 17, 18, 25):
        for _ in range(n // 4):
            text = digits(nd)
            cut = int(rng.integers(0, nd + 1))
            text = text[:cut] + "." + text[cut:] if 0 < cut < nd else text
            out.append(rng.choice(["", "-"]) + text)
    for _ in range(n // 2):                                                           # leading zeros count among the 17 digits
        out.append("0" * int(rng.integers(1, 20)) + digits(int(rng.integers(1, 20))) + "." + digits(int(rng.integers(1, 20))))
        out.append("0." + "0" * int(rng.integers(1, 25)) + digits(int(rng.integers(1, 20))))
    for _ in range(n):                                                                # exponent forms, both signs, both letters
        mant = digits(int(rng.integers(1, 20)))
        if rng.random() < 0.7:
            mant += "." + digits(int(rng.integers(1, 20)))
        out.append(rng.choice(["", "-"]) + mant + rng.choice(["e", "E"]) + rng.choice(["", "+", "-"]) + str(int(rng.integers(0, 280))))
    out += ["-0.0", "0.0", "-0", "0", "1e0", "1E-0", "5e-324", "1e-320", "1e-325", "2.2250738585072014e-308", "1.7976931348623157e308",
            "1.7976931348623157e+308", "12345678901234567890e-20", "0.000000000000000000001e21", "1e-300", "1e300", "1e+300",
            "1.2345678901234567e-300", "9.999999999999999e+299", "1e007", "1e0000"]
    return out


def test_random_field_texts_read_as_pandas_reads_them():
    texts = field_texts(5, 30000)
    assert len(texts) > 200000
    n = len(texts) // 5 * 5
    lines = ["{},{},{},{},{},{},{}".format(i, (i * 7) % 1000, *texts[5 * i:5 * i + 5]) for i in range(n // 5)]
    lines[3] = "4294967295,4294967295," + lines[3].split(",", 2)[2]
    lines[4] = "0000000007,000," + lines[4].split(",", 2)[2]
    data = (HEADER + "\n".join(lines) + "\n").encode()
    columns = served(data)
    assert columns[0][3] == 4294967295 and columns[0][4] == 7 and columns[1][4] == 0
    # what the bound of the power table must cover: every repr of a double in 1e-300 .. 1e300 was served above; and -0.0 is kept
    one = served((HEADER + "1,2,-0.0,-0,0.0,-0.0e5,-0e-3\n").encode())
    assert [np.signbit(one[k][0]) for k in range(2, 7)] == [True, True, False, True, True]


def test_permuted_and_extra_columns():
    from ysmr_amd.helper_file import rows_to_csv_bytes
    rows = st.value_mix_rows(3000)
    base = pd.read_csv(io.BytesIO(rows_to_csv_bytes(rows)), dtype=str)
    rng = np.random.default_rng(2)
    base["ILLUMINATION"] = [repr(float(v)) for v in rng.uniform(0, 255, len(base))]
    base["index"] = [str(v) for v in range(len(base))]
    base["note"] = rng.choice(["", "a b", "x;y", "nan", "-", "1e5", "+3", " 7 "], len(base))
    for order in (["index"] + NAMES, NAMES + ["ILLUMINATION"], ["note"] + NAMES[::-1] + ["index"],
                  ["DEGREES_ANGLE", "note", "TRACK_ID", "index", "WIDTH", "POSITION_Y", "ILLUMINATION", "POSITION_T", "HEIGHT", "POSITION_X"],
                  NAMES + ["note"]):
        text = base[order].to_csv(index=False, lineterminator="\n")
        served(text.encode())


GOOD = "1,2,3.5,4.5,5.5,6.5,7.5"

NOT_SERVED = {
    "empty line": "\n",
    "empty wanted field": "1,2,,4.5,5.5,6.5,7.5",
    "empty integer field": ",2,3.5,4.5,5.5,6.5,7.5",
    "empty last field": "1,2,3.5,4.5,5.5,6.5,",
    "nan": "1,2,nan,4.5,5.5,6.5,7.5",
    "NaN": "1,2,3.5,NaN,5.5,6.5,7.5",
    "inf": "1,2,3.5,4.5,inf,6.5,7.5",
    "-inf": "1,2,3.5,4.5,-inf,6.5,7.5",
    "Infinity": "1,2,3.5,4.5,5.5,Infinity,7.5",
    "leading plus": "1,2,+3.5,4.5,5.5,6.5,7.5",
    "leading plus on an integer": "+1,2,3.5,4.5,5.5,6.5,7.5",
    "leading blank": "1,2, 3.5,4.5,5.5,6.5,7.5",
    "trailing blank": "1,2,3.5 ,4.5,5.5,6.5,7.5",
    "blank before an integer": "1, 2,3.5,4.5,5.5,6.5,7.5",
    "no fraction digits": "1,2,1.,4.5,5.5,6.5,7.5",
    "no integer digits": "1,2,.5,4.5,5.5,6.5,7.5",
    "underscore": "1,2,3_5,4.5,5.5,6.5,7.5",
    "underscore in an integer": "1_0,2,3.5,4.5,5.5,6.5,7.5",
    "too few fields": "1,2,3.5,4.5,5.5,6.5",
    "too many fields": "1,2,3.5,4.5,5.5,6.5,7.5,8.5",
    "a trailing comma": "1,2,3.5,4.5,5.5,6.5,7.5,",
    "integer out of range": "4294967296,2,3.5,4.5,5.5,6.5,7.5",
    "integer of eleven digits": "00000000001,2,3.5,4.5,5.5,6.5,7.5",
    "negative integer": "1,-2,3.5,4.5,5.5,6.5,7.5",
    "integer with a fraction": "1,2.0,3.5,4.5,5.5,6.5,7.5",
    "integer with an exponent": "1e3,2,3.5,4.5,5.5,6.5,7.5",
    "exponent without digits": "1,2,3.5e,4.5,5.5,6.5,7.5",
    "exponent sign without digits": "1,2,3.5e+,4.5,5.5,6.5,7.5",
    "exponent beyond the table": "1,2,1e309,4.5,5.5,6.5,7.5",
    "exponent below the table": "1,2,1e-326,4.5,5.5,6.5,7.5",
    "exponent of five digits": "1,2,1e00001,4.5,5.5,6.5,7.5",
    "overflow": "1,2,9e308,4.5,5.5,6.5,7.5",
    "two signs": "1,2,--3.5,4.5,5.5,6.5,7.5",
    "two points": "1,2,3.5.1,4.5,5.5,6.5,7.5",
    "hexadecimal": "1,2,0x10,4.5,5.5,6.5,7.5",
    "a letter behind the number": "1,2,3.5f,4.5,5.5,6.5,7.5",
    "minus alone": "1,2,-,4.5,5.5,6.5,7.5",
}


@pytest.mark.parametrize("case", sorted(NOT_SERVED))
def test_what_is_not_served_is_counted_and_leaves_no_value(case):
    from ysmr_amd.helper_file import parse_csv_devicelike
    bad = NOT_SERVED[case]
    data = (HEADER + GOOD + "\n" + (bad if bad.endswith("\n") else bad + "\n") + GOOD + "\n").encode()
    columns, n, unserved, flags, _ = parse_csv_devicelike(data)
    assert (n, unserved, flags) == (3, 1, 0)
    assert columns[0][1] == 0xFFFFFFFF and columns[1][1] == 0xFFFFFFFF
    assert all(c.view(np.uint64)[1] == 0xFFFFFFFFFFFFFFFF for c in columns[2:])
    assert [float(c[0]) for c in columns] == [float(c[2]) for c in columns] == [1, 2, 3.5, 4.5, 5.5, 6.5, 7.5]
    # ... and as the last line, without its newline (the empty line: a file that ends in "\n\n")
    columns, n, unserved, flags, _ = parse_csv_devicelike((HEADER + GOOD + "\n" + bad).encode())
    assert (n, unserved, flags) == (2, 1, 0)
    assert columns[0][1] == 0xFFFFFFFF and columns[2].view(np.uint64)[1] == 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("byte,flag", [(b'"', 1), (b"\r", 2), (b"\x00", 4), (b"\xc3\xa4", 4)])
def test_quotes_carriage_returns_and_bytes_that_are_not_plain_are_flagged(byte, flag):
    from ysmr_amd.helper_file import parse_csv_devicelike
    header = (",".join(NAMES + ["note"]) + "\n").encode()
    data = header + GOOD.encode() + b",a" + byte + b"b\n"
    assert parse_csv_devicelike(data)[3] == flag
    assert parse_csv_devicelike(header + GOOD.encode() + b",ab\n")[3] == 0
    if byte == b"\r":
        assert parse_csv_devicelike((HEADER + GOOD + "\r\n").encode())[2:4] == (1, 2)


@pytest.mark.parametrize("header", ["TRACK_ID,POSITION_T,POSITION_X,POSITION_Y,WIDTH,HEIGHT",
                                    HEADER.strip() + ",TRACK_ID", HEADER.strip().replace("WIDTH", "width"),
                                    HEADER.strip().replace("HEIGHT", " HEIGHT"), "", "a,b,c,d,e,f,g,h"])
def test_a_header_without_the_seven_names_or_with_one_twice_is_refused(header):
    from ysmr_amd.helper_file import csv_header_plan, parse_csv_devicelike
    assert csv_header_plan(header.encode()) is None
    assert parse_csv_devicelike((header + "\n" + GOOD + "\n").encode()) is None


def test_header_positions():
    from ysmr_amd.helper_file import csv_header_plan
    assert csv_header_plan(HEADER.strip().encode()) == (7, [0, 1, 2, 3, 4, 5, 6])
    assert csv_header_plan(("index," + HEADER.strip() + ",ILLUMINATION").encode()) == (9, [1, 2, 3, 4, 5, 6, 7])
    assert csv_header_plan(",".join(NAMES[::-1]).encode()) == (7, [6, 5, 4, 3, 2, 1, 0])
