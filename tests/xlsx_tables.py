"""Tables and csv files for the tests of the collated workbook (csrc/xlsx.hip, csrc/csv.hip: ysmr_csv_column_kinds), shared by
the CPU and the GPU tests: the tables whose sheet rows the device printer's host twin and its kernels must print as
``sheet_xml_host`` does, and the files whose column kinds must be pandas' dtypes or a refusal."""
import io
import re

import numpy as np
import pandas as pd

import table_csv_tables as tt

LAST_SHEET_ROW = 1048576


def finite_or_nan(df):
    """The infinities of a table's float64 columns replaced: ``inf`` is the one cell the two paths write differently (an inline
    string on the host, which alone ever meets one)."""
    out = df.copy()
    for name in out.columns:
        if out[name].dtype == np.float64:
            v = out[name].to_numpy().copy()
            v[np.isinf(v)] = 1.25
            out[name] = v
    return out


def mixed(n, seed=1):
    """All five column types, float64 cells steady, wide (1e-14-sized, 1e300, subnormals), NaN, both zeros; int64 at its
    widest served magnitudes."""
    shape = (("u", np.uint32), ("i", np.int64), ("f", np.float64), ("j", np.int32), ("b", np.int8), ("g", np.float64), ("h", np.float64))
    df = finite_or_nan(tt.shaped(shape, n, seed=seed, wide="some"))
    if n >= 5:
        df.loc[0, "i"], df.loc[1, "i"] = 999999999999999999, -999999999999999999
        df.loc[0, "f"], df.loc[1, "f"], df.loc[2, "f"], df.loc[3, "f"] = -0.0, 1e300, 5e-324, 1e-14
        df.loc[4, ["f", "g", "h"]] = np.nan                          # every float of the row, with the integers beside them
    return df


def only_floats(n, seed=2, wide="some"):
    df = finite_or_nan(tt.shaped((("x", np.float64), ("y", np.float64), ("z", np.float64)), n, seed=seed, wide=wide))
    if n >= 3:
        df.iloc[1, :] = np.nan                                        # a row of only NaN
        df["y"] = np.nan                                              # a column of only NaN
    return df


def widest_sixteen(n):
    """Sixteen float64 columns of 24-byte values: with a sheet row of seven digits a row is as long as the plan's longest."""
    return tt.uniform_rows((np.float64,) * 16, n, lambda r: True)


def host_body(df, first_row):
    """The rows of ``sheet_xml_host`` without the head, the header row and the closing tags."""
    from ysmr_amd import helper_file as hf
    xml = hf.sheet_xml_host(df, first_row)
    head = hf.sheet_prefix([str(k) for k in df.columns], first_row - 1)
    assert xml.startswith(head) and xml.endswith(hf._SHEET_SUFFIX)
    return xml[len(head):len(xml) - len(hf._SHEET_SUFFIX)]


def without_index(body):
    """The rows of a sheet without column A, every other column a letter to the left: what ``with_index = 0`` prints."""
    body = re.sub(rb'<c r="A\d+" s="1"><v>\d+</v></c>', b"", body)
    return re.sub(rb'<c r="([B-Q])(\d+)"', lambda m: b'<c r="' + bytes([m.group(1)[0] - 1]) + m.group(2) + b'"', body)


# ---- files for the kinds -------------------------------------------------------------------------------------------------------
def _file(rows, header="a,b,c", last_newline=True):
    text = header + "\n" + "\n".join(rows) + "\n"
    return (text if last_newline else text[:-1]).encode()


# (lines of 14 bytes and more: the index pass keeps a table of line starts sized for the track tables' lines, and a file with
# more lines than its bytes / 14 is one it refuses -- such a file is the host path's)
BASE_ROWS = ["1001,2.500000001,-3003", "4004,0.125000001,6006", "-7007,1.00000001e-5,9009", "10010,11.00000000,12012", "13013,-2.75000001,15015"]


def kinds_files():
    """``name -> (bytes, n_columns, served)``: ``served`` says whether the reader must take the file (then with pandas' dtypes)
    or refuse it.  The one field that changes a column's kind stands in the first line, in the last, or in a last line without
    its newline."""
    files = {"plain": (_file(BASE_ROWS), 3, True)}
    deciding = {"a float among ints": ("1.5", True), "an empty field": ("", True), "a string": ("x", False),
                "nineteen digits": ("1234567890123456789", False), "a point and nothing": ("1.", False), "a plus": ("+1", False),
                "nan": ("nan", False), "eighteen digits": ("-999999999999999999", True)}
    for what, (field, served) in deciding.items():
        for where in ("first", "last", "last, no newline"):
            rows = list(BASE_ROWS)
            k = 0 if where == "first" else len(rows) - 1
            parts = rows[k].split(",")
            parts[0] = field
            rows[k] = ",".join(parts)
            files["{} in the {} line".format(what, where)] = (_file(rows, last_newline=where != "last, no newline"), 3, served)
    for where, k in (("first", 0), ("last", len(BASE_ROWS) - 1)):
        few, many = list(BASE_ROWS), list(BASE_ROWS)
        few[k] = "1001,2.500000001"
        many[k] = "1001,2.500000001,3003,4004"
        files["too few fields in the {} line".format(where)] = (_file(few), 3, False)
        files["too many fields in the {} line".format(where)] = (_file(many), 3, False)
    files["a column of only empty fields"] = (_file(["100001,,300003", "400004,,600006"]), 3, True)
    files["an empty line"] = (_file(["100000000000001", "", "300000000000003"], header="a"), 1, False)
    files["an exponent beyond the table"] = (_file(["100001,1e400,300003"]), 3, False)
    return files


def long_lines_file(deciding_row, n_rows, field="x"):
    """Sixteen float columns of 20-byte fields: 256 such lines are more than twice the parse's staged span, so the later
    lines of a workgroup are read from global memory.  Column 5 of ``deciding_row`` holds ``field``."""
    rng = np.random.default_rng(5)
    values = rng.uniform(1.0, 2.0, (n_rows, 16))
    rows = [",".join("{:.18f}".format(v) for v in line) for line in values]
    parts = rows[deciding_row].split(",")
    parts[5] = field
    rows[deciding_row] = ",".join(parts)
    return _file(rows, header=",".join("c{}".format(k) for k in range(16)))


def pandas_dtypes(data):
    """pandas' dtypes of the file and its row count, as the collation's host path reads it."""
    df = pd.read_csv(io.StringIO(data.decode("utf-8")), sep=",", header=0)
    return [df.iloc[:, k].dtype for k in range(df.shape[1])], len(df)
