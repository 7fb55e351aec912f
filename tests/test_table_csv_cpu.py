"""The device csv writer's host form (``ysmr_table_format_devicelike``: the arithmetic of csrc/fmt.h and the rules of
csrc/table_csv.hip a row at a time) against the installed pandas: the bytes of ``DataFrame.to_csv(index=False)``, no tolerance.
Then the declarations, the argument checks and the bound.  Needs the built library and no GPU."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

import table_csv_tables as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3


def devicelike(df, header=None):
    from ysmr_amd import helper_file
    return helper_file.table_csv_devicelike(df, header=header)


def wide_count(df):
    return int(sum(tt.is_wide(df[c]).sum() for c in df.columns if df[c].dtype == np.float64))


@pytest.mark.parametrize("dtype", tt.TYPES)
def test_every_column_type_alone(dtype):
    df = tt.shaped((("only", dtype),), 3000, seed=1)
    got, wide = devicelike(df)
    assert got == tt.pandas_bytes(df)
    assert wide == wide_count(df)


def test_integer_extremes():
    df = pd.DataFrame({"a": np.array([-9223372036854775808, 9223372036854775807, 0, -1, 10 ** 18], np.int64),
                       "b": np.array([4294967295, 0, 9, 10, 4294967294], np.uint32),
                       "c": np.array([-2147483648, 2147483647, 0, -1, 99], np.int32),
                       "d": np.array([-128, 127, 0, -1, 100], np.int8)})
    got, wide = devicelike(df)
    assert got == tt.pandas_bytes(df) and wide == 0
    assert got.split(b"\n")[1] == b"-9223372036854775808,4294967295,-2147483648,-128"


def test_sixteen_columns():
    shape = tuple(("k{}".format(k), tt.TYPES[k % 5]) for k in range(16))
    df = tt.shaped(shape, 2000, seed=2)
    got, wide = devicelike(df)
    assert got == tt.pandas_bytes(df) and wide == wide_count(df) > 0


@pytest.mark.parametrize("wide", ("none", "some", "all"))
@pytest.mark.parametrize("shape", ("selected", "analysed"))
def test_the_selected_and_the_analysed_shape(shape, wide):
    df = tt.shaped(tt.SELECTED if shape == "selected" else tt.ANALYSED, 20000, seed=4, wide=wide)
    floats = np.concatenate([df[c].to_numpy() for c in df.columns if df[c].dtype == np.float64])
    if wide != "all":
        assert np.isnan(floats).any() and np.isposinf(floats).any() and np.isneginf(floats).any()
        assert ((floats == 0) & np.signbit(floats)).any() and ((floats == 0) & ~np.signbit(floats)).any()
    if wide != "none":
        a = np.abs(floats[np.isfinite(floats)])
        assert ((a > 0) & (a < 1e-13)).any() and (a > 1e299).any(), "1e-14-sized and 1e300-sized cells"
    ints = df[[c for c in df.columns if df[c].dtype == np.int64]].to_numpy()
    if ints.size:
        assert ints.min() == np.iinfo(np.int64).min and ints.max() == np.iinfo(np.int64).max
    small = df[[c for c in df.columns if df[c].dtype == np.int8]].to_numpy()
    if small.size:
        assert small.min() == -128 and small.max() == 127
    got, counted = devicelike(df)
    assert got == tt.pandas_bytes(df)
    assert counted == wide_count(df)
    assert (counted == 0) == (wide == "none")


@pytest.mark.parametrize("n", (0, 1))
def test_no_row_and_one_row(n):
    for shape in (tt.SELECTED, tt.ANALYSED):
        df = tt.shaped(shape, n, seed=6, wide="all")
        assert devicelike(df)[0] == tt.pandas_bytes(df)


def test_an_empty_header_and_a_long_one():
    df = tt.shaped(tt.ANALYSED, 300, seed=8)
    whole = tt.pandas_bytes(df)
    body = whole[whole.index(b"\n") + 1:]
    assert devicelike(df, header=b"")[0] == body
    long_header = ("h" * 299 + "\n").encode()
    assert len(long_header) == 300 and devicelike(df, header=long_header)[0] == long_header + body
    renamed = df.rename(columns={name: "{}_{}".format(name, "n" * 12) for name in df.columns})     # ... and one pandas writes
    assert len(tt.pandas_bytes(renamed).split(b"\n")[0]) > 300 - 1
    assert devicelike(renamed)[0] == tt.pandas_bytes(renamed)
    assert devicelike(df.iloc[:0], header=b"") == (b"", 0)


def test_frames_the_writer_leaves_to_pandas():
    from ysmr_amd import helper_file
    base = tt.shaped(tt.SELECTED, 5, seed=9)
    assert helper_file.table_csv_plan(base) is not None
    for frame in (base.assign(WIDTH=base["WIDTH"].astype(np.float32)), base.assign(note="x"), base.rename(columns={"WIDTH": "a,b"}),
                  base.rename(columns={"WIDTH": 'a"b'}), base.rename(columns={"WIDTH": "a\nb"}), base.rename(columns={"WIDTH": "a\rb"}),
                  base.rename(columns={"WIDTH": ""}), base.rename(columns={"WIDTH": 7}), base.iloc[:, :0],
                  base.assign(TRACK_ID=base["TRACK_ID"].astype("UInt32")), base.assign(POSITION_T=base["POSITION_T"].astype(np.uint16)),
                  pd.DataFrame({"c{}".format(k): np.arange(3, dtype=np.int64) for k in range(17)})):
        assert helper_file.table_csv_plan(frame) is None, list(frame.columns)
    plain = base.rename(columns={"WIDTH": "Länge (µm)"})
    assert devicelike(plain)[0] == tt.pandas_bytes(plain)


def _columns(dtypes, arrays):
    from ysmr_amd import helper_file
    return helper_file._table_columns([a.ctypes.data for a in arrays], dtypes)


def test_the_bound_is_reached_and_never_exceeded_on_all_widest_rows():
    from ysmr_amd import _lib
    L = _lib.lib()
    for dtypes in ((np.float64,) * 16, tt.TYPES, tt.TYPES * 3 + (np.uint32,), (np.int8,)):
        n = 700
        df = tt.uniform_rows(dtypes, n, lambda k: True)
        arrays = [np.ascontiguousarray(df.iloc[:, k].to_numpy()) for k in range(len(dtypes))]
        cols = _columns(dtypes, arrays)
        header = (",".join(df.columns) + "\n").encode()
        line = sum(tt.WIDTH[dt] + 1 for dt in dtypes)
        bound = L.ysmr_table_csv_bound(n, len(dtypes), cols, len(header))
        assert bound == len(header) + n * line
        got, _ = devicelike(df)
        assert got == tt.pandas_bytes(df) and len(got) == bound
        # a capacity one byte short
        out = np.full(bound + 64, 0xA5, np.uint8)
        length, wide = ctypes.c_size_t(0), ctypes.c_longlong(0)
        rc = L.ysmr_table_format_devicelike(n, len(dtypes), cols, header, len(header), out.ctypes.data, bound - 1, ctypes.byref(length),
                                            ctypes.byref(wide))
        assert rc == ERR_CAPACITY and b"too small" in L.ysmr_last_error()
        assert (out == 0xA5).all()
        rc = L.ysmr_table_format_devicelike(n, len(dtypes), cols, header, len(header), out.ctypes.data, bound, ctypes.byref(length),
                                            ctypes.byref(wide))
        assert rc == OK and length.value == bound and (out[bound:] == 0xA5).all()


def test_argument_checks():
    from ysmr_amd import _lib
    L = _lib.lib()
    values = np.arange(4, dtype=np.float64)
    cols = _columns([np.float64], [values])
    out = np.zeros(4096, np.uint8)
    length, wide = ctypes.c_size_t(0), ctypes.c_longlong(0)

    def call(n=4, n_columns=1, columns=cols, header=b"v\n", header_bytes=2, buffer=out.ctypes.data, capacity=4096, length_p=ctypes.byref(length),
             wide_p=ctypes.byref(wide)):
        return L.ysmr_table_format_devicelike(n, n_columns, columns, header, header_bytes, buffer, capacity, length_p, wide_p)
    assert call() == OK and out[:length.value].tobytes() == b"v\n0.0\n1.0\n2.0\n3.0\n"
    assert call(columns=None) == ERR_ARG
    assert call(buffer=None) == ERR_ARG
    assert call(length_p=None) == ERR_ARG
    assert call(wide_p=None) == ERR_ARG
    assert call(header=None) == ERR_ARG
    assert call(header=None, header_bytes=0) == OK
    assert call(n=-1) == ERR_ARG
    assert call(n_columns=0) == ERR_ARG
    many = (_lib.TableColumn * 17)(*([cols[0]] * 17))
    assert call(n_columns=17, columns=many) == ERR_ARG and b"1..16" in L.ysmr_last_error()
    assert call(n_columns=16, columns=many) == OK
    unknown = (_lib.TableColumn * 1)()
    unknown[0].data, unknown[0].type = values.ctypes.data, 5
    assert call(columns=unknown) == ERR_ARG and b"unknown type" in L.ysmr_last_error()
    unknown[0].type = -1
    assert call(columns=unknown) == ERR_ARG
    null = (_lib.TableColumn * 1)()
    null[0].data, null[0].type = None, 4
    assert call(columns=null) == ERR_ARG
    assert call(n=0, columns=null) == OK and length.value == 2
    # the same rules in the device entry, before anything is launched (no GPU is touched by a refused call)
    dev = lambda **kw: L.ysmr_table_format_device(None, kw.get("n", 4), kw.get("n_columns", 1), kw.get("columns", cols), b"v\n", 2, 1, 1 << 20,  # noqa: E731
                                                  kw.get("csv", 1), kw.get("capacity", 4096), kw.get("length", 1), kw.get("wide", 1))
    assert dev(n_columns=0) == ERR_ARG and dev(n_columns=17, columns=many) == ERR_ARG and dev(columns=unknown) == ERR_ARG
    assert dev(columns=None) == ERR_ARG and dev(csv=None) == ERR_ARG and dev(length=None) == ERR_ARG and dev(wide=None) == ERR_ARG
    assert dev(n=-1) == ERR_ARG
    assert dev(capacity=2 + 4 * 25 - 1) == ERR_CAPACITY
    assert dev(n=2 ** 40) == ERR_CAPACITY


def test_what_the_plan_refuses():
    from ysmr_amd import _lib
    L = _lib.lib()
    cols = (_lib.TableColumn * 16)()
    for k in range(16):
        cols[k].data, cols[k].type = None, 4
    line = 16 * 25
    most = (2 ** 32 - 1) // line
    assert L.ysmr_table_csv_bound(most, 16, cols, 0) == most * line
    assert L.ysmr_table_csv_bound(most, 16, cols, (2 ** 32 - 1) - most * line) == 2 ** 32 - 1
    assert L.ysmr_table_csv_bound(most, 16, cols, 2 ** 32 - most * line) == 0
    assert L.ysmr_table_csv_bound(most + 1, 16, cols, 0) == 0
    assert L.ysmr_table_csv_bound(-1, 16, cols, 0) == 0
    assert L.ysmr_table_csv_bound(1, 16, cols, 2 ** 64 - 1) == 0
    assert L.ysmr_table_csv_bound(2 ** 62, 16, cols, 0) == 0
    assert L.ysmr_table_csv_bound(0, 16, cols, 77) == 77
    assert L.ysmr_table_csv_bound(1, 0, cols, 0) == 0 and L.ysmr_table_csv_bound(1, 17, cols, 0) == 0 and L.ysmr_table_csv_bound(1, 1, None, 0) == 0
    assert L.ysmr_table_format_workspace_bytes(0, 16, cols) == 256
    for n in (1, 127, 128, 129, 10 ** 6, most):
        total = L.ysmr_table_format_workspace_bytes(n, 16, cols)
        assert total % 256 == 0 and total >= n * (line + 16 * 25 + 4), n
    for n in (-1, most + 1, 2 ** 62):
        assert L.ysmr_table_format_workspace_bytes(n, 16, cols) == 0
    cols[3].type = 9
    assert L.ysmr_table_csv_bound(1, 16, cols, 0) == 0 and L.ysmr_table_format_workspace_bytes(1, 16, cols) == 0


def test_declarations_and_the_abi_number():
    from ysmr_amd import _lib
    header = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    assert re.search(r"#define\s+YSMR_ABI_VERSION\s+15\b", header) and _lib.lib().ysmr_abi_version() == 15 == _lib.ABI_VERSION
    for k, name in enumerate(("U32", "I64", "I32", "I8", "F64")):
        assert re.search(r"#define\s+YSMR_COL_{}\s+{}\b".format(name, k), header)
    assert "typedef struct { const void *data; int32_t type; int32_t reserved; } ysmr_table_column;" in header
    flat = " ".join(header.split())
    for declaration in (
            "size_t ysmr_table_csv_bound(long long n_rows, int n_columns, const ysmr_table_column *columns, size_t header_bytes);",
            "size_t ysmr_table_format_workspace_bytes(long long n_rows, int n_columns, const ysmr_table_column *columns);",
            "int ysmr_table_format_device(void *stream, long long n_rows, int n_columns, const ysmr_table_column *columns, "
            "const char *header_host, size_t header_bytes, void *workspace_dev, size_t workspace_bytes, char *csv_dev, "
            "size_t csv_capacity, unsigned long long *csv_length_dev, uint32_t *wide_cells_dev);",
            "void ysmr_table_format_geometry(int *rows_per_group, int *staged_bytes);",
            "int ysmr_table_format_devicelike(long long n_rows, int n_columns, const ysmr_table_column *columns, const char *header, "
            "size_t header_bytes, char *out, size_t out_capacity, size_t *out_length, long long *wide_cells);",
            "int ysmr_fmt_f64_text(const double *values, long long n, int printer, char *slots, uint8_t *lengths);"):
        assert declaration in flat, declaration
    for name in ("ysmr_table_csv_bound", "ysmr_table_format_workspace_bytes", "ysmr_table_format_device", "ysmr_table_format_geometry",
                 "ysmr_table_format_devicelike", "ysmr_fmt_f64_text"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert ctypes.sizeof(_lib.TableColumn) == 16
    rows, staged = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_table_format_geometry(ctypes.byref(rows), ctypes.byref(staged))
    assert rows.value % 64 == 0 and staged.value == rows.value * 16 * 25 <= 65536
