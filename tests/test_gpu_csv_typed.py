"""``read_typed_device`` (``ysmr_csv_index`` + ``ysmr_csv_parse_typed``, csrc/csv.hip) on the device against the installed
``pandas.read_csv(usecols, dtype)``: every column bit for bit (NaN positions included), ``path_taken == 'device'`` and no row
unserved -- so the host path cannot hide a wrong kernel -- at the row counts around a workgroup's lines, with a line longer
than the staged span, a last line without its newline, the columns in another order; and the files that must NOT be served."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch        # before the library is loaded: both then share torch's HIP runtime, as in test_gpu_table_csv.py

import analysed_tables as at

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def geometry():
    from ysmr_amd import _lib
    rows, span = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_csv_geometry(None, ctypes.byref(rows), ctypes.byref(span))
    return rows.value, span.value


def read(tmp_path, data, fields=at.FIELDS, **kwargs):
    from ysmr_amd.helper_file import read_typed_device
    path = tmp_path / "table_analysed.csv"
    path.write_bytes(data)
    return read_typed_device(str(path), fields, "cuda:0", **kwargs)


def assert_served_as_pandas(tmp_path, data, fields=at.FIELDS):
    import io
    table = read(tmp_path, data, fields)
    assert table.path_taken == "device" and table.unserved == 0 and table.flags == 0, (table.path_taken, table.unserved, table.flags)
    dtype = {f[0]: f[1] for f in fields}
    ref = pd.read_csv(io.BytesIO(data), sep=",", header=0, usecols=list(dtype), dtype=dtype)
    assert table.n_rows == len(ref) == len(table)
    assert sorted(table.columns) == sorted(dtype)
    for name, kind in dtype.items():
        got = table.columns[name].cpu().numpy()
        want = ref[name].to_numpy()
        assert want.dtype == np.dtype(kind) and len(got) == len(want), name
        width = {1: np.uint8, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        diff = np.flatnonzero(got.view(width) != want.view(width))
        assert len(diff) == 0, "{}: {} of {} differ, first at row {}: {!r} against pandas' {!r}".format(
            name, len(diff), len(want), diff[0], got[diff[0]], want[diff[0]])
    return table


def row_counts():
    rows, _span = geometry()
    return [0, 1, rows - 1, rows, rows + 1, 3 * rows + 1]


@pytest.mark.parametrize("k", range(6))
def test_row_counts_around_a_workgroups_lines(tmp_path, k):
    n = row_counts()[k]
    table = assert_served_as_pandas(tmp_path, at.csv_bytes(at.analysed(n, seed=k)))
    assert table.n_rows == n
    if n > 100:
        assert int(table.columns["POSITION_X"].isnan().sum()) > 0           # (empty cells were read)


def test_a_last_line_without_its_newline(tmp_path):
    rows, _span = geometry()
    for n in (1, rows + 1):
        data = at.csv_bytes(at.analysed(n, seed=7), last_newline=False)
        assert not data.endswith(b"\n")
        assert assert_served_as_pandas(tmp_path, data).n_rows == n


def test_a_line_longer_than_the_staged_span_is_parsed_from_global_memory(tmp_path):
    rows, span = geometry()
    df = at.analysed(rows + 40, seed=3)
    df.insert(5, "note", "x")
    long_bytes = max(50_000, span + 1000)
    df.loc[17, "note"] = "y" * long_bytes                 # in the first workgroup: the lines behind it lie beyond its span
    df.loc[rows + 5, "note"] = "z" * long_bytes           # ... and the second workgroup's span ends inside this one
    data = at.csv_bytes(df)
    assert len(data) > 2 * long_bytes
    assert_served_as_pandas(tmp_path, data)


def test_columns_in_another_order_with_extra_columns_and_fewer_fields(tmp_path):
    rows, _span = geometry()
    df = at.analysed(rows + 3, seed=4)
    df["extra_text"] = "a b;c"
    df["extra_empty"] = np.nan
    df = df[["extra_empty", "turn_points", "POSITION_Y", "extra_text", "motility_phenotype", "WIDTH", "moving", "TRACK_ID", "HEIGHT",
             "POSITION_X", "DEGREES_ANGLE", "POSITION_T", "angle_diff", "tp_of_tracks", "travelled_dist"]]
    data = at.csv_bytes(df)
    assert_served_as_pandas(tmp_path, data)
    assert_served_as_pandas(tmp_path, data, [f for f in at.FIELDS if f[0] != "motility_phenotype"])
    # the other types of the reader, on the same text: int32 and float64 ids, an int64 flag
    assert_served_as_pandas(tmp_path, data, [("POSITION_T", np.int32), ("TRACK_ID", np.float64), ("moving", np.int64), ("tp_of_tracks", np.float64, True)])


def test_the_thirteen_columns_of_an_analysed_csv_with_empty_cells(tmp_path):
    df = at.analysed(1500, seed=5, nan_share=0.2)
    assert list(df.columns) == at.ROW_COLUMNS and df["tp_of_tracks"].isna().any() and df["POSITION_X"].isna().any()
    table = assert_served_as_pandas(tmp_path, at.csv_bytes(df))
    # ... which is what annotate_video's own pandas read holds
    ref = at.pandas_columns(at.csv_bytes(df))
    assert np.array_equal(table.columns["TRACK_ID"].cpu().numpy().view(np.uint32).astype(np.int64), ref["TRACK_ID"].to_numpy())
    phenotype = pd.to_numeric(ref["motility_phenotype"], errors="coerce").to_numpy(dtype=np.float64)
    assert np.array_equal(table.columns["motility_phenotype"].cpu().numpy(), phenotype)


def test_a_name_pandas_would_demand_has_to_be_in_the_header(tmp_path):
    df = at.analysed(20, seed=6).drop(columns=["motility_phenotype"])
    fields = [f for f in at.FIELDS if f[0] != "motility_phenotype"]
    assert read(tmp_path, at.csv_bytes(df), fields).path_taken == "device"
    assert read(tmp_path, at.csv_bytes(df), fields, also_in_header=("motility_phenotype",)).path_taken == "host"


def test_files_that_are_not_served_go_to_the_host(tmp_path):
    df = at.analysed(300, seed=8, nan_share=0.0)
    good = at.csv_bytes(df)
    assert read(tmp_path, good).path_taken == "device"
    lines = good.split(b"\n")
    x = at.ROW_COLUMNS.index("POSITION_X")
    cells = lines[200].split(b",")
    cells[x] = b"nan"
    table = read(tmp_path, b"\n".join(lines[:200] + [b",".join(cells)] + lines[201:]))
    assert (table.path_taken, table.unserved, table.columns) == ("host", 1, None)
    cells = lines[290].split(b",")
    cells[at.ROW_COLUMNS.index("moving")] = b"128"
    table = read(tmp_path, b"\n".join(lines[:290] + [b",".join(cells)] + lines[291:]))
    assert (table.path_taken, table.unserved) == ("host", 1)
    # a hand-made file of short lines: the index pass, sized for lines of 14 bytes and more, flags it
    from ysmr_amd.helper_file import CSV_FLAG_TOO_MANY_LINES
    short = (",".join(f[0] for f in at.FIELDS) + "\n" + "1,2,,,0,0,0\n" * 400).encode()
    table = read(tmp_path, short)
    assert table.path_taken == "host" and table.flags & CSV_FLAG_TOO_MANY_LINES
    # ... which pandas reads
    assert len(at.pandas_columns(short)) == 400
