"""The collated workbook on the GPU: ``ysmr_xlsx_sheet_device`` (csrc/xlsx.hip) against its host twin byte for byte at the row
counts where its kernels change what they do (a workgroup ``R`` of ``ysmr_xlsx_sheet_geometry``, several workgroups, one row,
none), at the sheet's last rows, with wide and NaN cells and without the index column; ``ysmr_csv_column_kinds`` (csrc/csv.hip)
against its twin on the CPU test's files and on files whose deciding field lies beyond the staged span and in the second
workgroup; then ``collate_results_csv_to_xlsx`` on a folder with a statistics file written by ``evaluate_tracks``, an analysed
csv with empty cells and a csv with a string column: the device path's workbook is the host path's, byte for byte."""
import ctypes
import logging
import os

import numpy as np
import pandas as pd
import pytest
import torch        # before the library is loaded: both then share torch's HIP runtime, as in test_gpu_pipeline.py

import analysed_tables as at
import select_tables as st
import xlsx_tables as xt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def geometry():
    from ysmr_amd import _lib
    rows, staged, longest = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_xlsx_sheet_geometry(ctypes.byref(rows), ctypes.byref(staged), ctypes.byref(longest))
    return rows.value, staged.value, longest.value


def upload(df):
    tensors = []
    for k in range(df.shape[1]):
        values = np.ascontiguousarray(df.iloc[:, k].to_numpy())
        tensors.append(torch.from_numpy(values.view(np.int32) if values.dtype == np.uint32 else values).to(DEV))
    return tensors


def device_sheet(df, first_row=2, with_index=True, prefix=None, suffix=None):
    """(text, wide cells) of the device printer for a DataFrame of the five dtypes; the reported length is the text's."""
    from ysmr_amd import helper_file as hf
    dtypes = hf.table_csv_plan(df)[1]
    prefix = hf.sheet_prefix(list(df.columns), first_row - 1) if prefix is None else prefix
    suffix = hf._SHEET_SUFFIX if suffix is None else suffix
    xml, length, wide = hf.xlsx_sheet_device(upload(df), dtypes, len(df), first_row, with_index, prefix, suffix, torch.device(DEV))
    return xml[:length].cpu().numpy().tobytes(), wide


def twin_sheet(df, first_row=2, with_index=True, prefix=None, suffix=None):
    from ysmr_amd import helper_file as hf
    return hf.xlsx_sheet_devicelike(df, first_row=first_row, with_index=with_index, prefix=prefix, suffix=suffix)


#: the row counts, R being the rows per workgroup (the library is asked when a test runs: it may not be built at collection)
ROW_COUNTS = ("0", "1", "R - 1", "R", "R + 1", "2 * R + 1")


@pytest.mark.parametrize("count", ROW_COUNTS)
def test_the_device_prints_what_its_twin_prints_at_the_kernels_row_counts(count):
    from ysmr_amd import helper_file as hf
    n = eval(count, {"R": geometry()[0]})
    df = xt.mixed(n, seed=n + 3)
    got, wide = device_sheet(df)
    assert (got, wide) == twin_sheet(df)
    assert got == hf.sheet_xml_host(df), "and both the host path's sheet"
    assert device_sheet(df) == (got, wide), "two calls give the same bytes"
    if n > 60:
        assert wide > 0 and b"</row><row r=\"6\"><c r=\"A6\" s=\"1\"><v>4</v></c><c r=\"B6\">" in got
    bare = device_sheet(df, prefix=b"", suffix=b"")
    assert bare == twin_sheet(df, prefix=b"", suffix=b"") and bare[0] == xt.host_body(df, 2)


@pytest.mark.parametrize("with_index", (True, False))
def test_sixteen_widest_columns_at_the_sheets_last_rows(with_index):
    df = xt.widest_sixteen(7)
    got, wide = device_sheet(df, first_row=1048570, with_index=with_index, prefix=b"", suffix=b"")
    assert (got, wide) == twin_sheet(df, first_row=1048570, with_index=with_index, prefix=b"", suffix=b"") and wide == 7 * 16
    body = xt.host_body(df, 1048570)
    assert got == (body if with_index else xt.without_index(body))
    assert got.endswith(b'1048576"><v>-1.2345678901234567e-308</v></c></row>')


@pytest.mark.parametrize("table", ("mixed", "only floats", "all wide"))
def test_without_the_index_column_and_with_rows_and_columns_of_only_nan(table):
    r = geometry()[0]
    n = 2 * r + 1
    df = {"mixed": lambda: xt.mixed(n, seed=8), "only floats": lambda: xt.only_floats(n), "all wide": lambda: xt.only_floats(n, wide="all")}[table]()
    for with_index in (True, False):
        got = device_sheet(df, first_row=99, with_index=with_index, prefix=b"<x>", suffix=b"</x>")
        assert got == twin_sheet(df, first_row=99, with_index=with_index, prefix=b"<x>", suffix=b"</x>")
        body = xt.host_body(df, 99)
        assert got[0] == b"<x>" + (body if with_index else xt.without_index(body)) + b"</x>"


def test_the_widest_rows_fill_the_staging_of_several_workgroups():
    """Sixteen widest float64 columns over 2 R + 1 rows that end at the sheet's last row: every workgroup's staging holds rows of
    the longest kind the geometry is sized for (the index has fewer digits than a full sheet's: the rows stay below it)."""
    r, staged, longest = geometry()
    n = 2 * r + 1
    df = xt.widest_sixteen(n)
    first = xt.LAST_SHEET_ROW - n + 1
    got = device_sheet(df, first_row=first, prefix=b"", suffix=b"")
    assert got == twin_sheet(df, first_row=first, prefix=b"", suffix=b"")
    assert got[0] == xt.host_body(df, first) and longest - 6 < len(got[0]) / n <= longest and r * longest <= staged


def _raw_call(df, first_row, capacity_less, fill=0xA5):
    from ysmr_amd import _lib, helper_file as hf
    L = _lib.lib()
    dtypes = hf.table_csv_plan(df)[1]
    tensors = upload(df)
    cols = hf._table_columns([t.data_ptr() for t in tensors], dtypes)
    n, prefix, suffix = len(df), b"<sheetData>", b"</sheetData>"
    bound = int(L.ysmr_xlsx_sheet_bound(n, len(dtypes), cols, first_row, 1, len(prefix), len(suffix)))
    ws_bytes = int(L.ysmr_xlsx_sheet_workspace_bytes(n, len(dtypes), cols, first_row, 1, len(suffix)))
    assert bound > 0 and ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    xml = torch.full((bound + 256,), fill, dtype=torch.uint8, device=DEV)
    meta = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    rc = L.ysmr_xlsx_sheet_device(_lib.stream_ptr(torch.device(DEV)), n, len(dtypes), cols, first_row, 1, prefix, len(prefix), suffix, len(suffix),
                                  ws.data_ptr(), ws_bytes, xml.data_ptr(), bound - capacity_less, meta.data_ptr(), meta[1:].data_ptr())
    torch.cuda.synchronize()
    return rc, xml.cpu().numpy(), meta.tolist(), bound, L.ysmr_last_error()


def test_nothing_is_written_behind_the_reported_length():
    r = geometry()[0]
    df = xt.mixed(2 * r + 1, seed=12)                      # (rows far shorter than the bound: a wide band between length and bound)
    rc, xml, meta, bound, _ = _raw_call(df, 2, 0)
    assert rc == 0
    length = meta[0]
    expect = twin_sheet(df, prefix=b"<sheetData>", suffix=b"</sheetData>")
    assert 0 < length < bound and length == len(expect[0]) and meta[1] & 0xFFFFFFFF == expect[1]
    assert xml[:length].tobytes() == expect[0]
    assert (xml[length:] == 0xA5).all(), "nothing behind the reported length"
    assert (_raw_call(df, 2, 0, fill=0x5A)[1][length:] == 0x5A).all()


def test_a_capacity_below_the_bound_is_refused_and_nothing_is_launched():
    df = xt.mixed(geometry()[0] + 1, seed=13)
    rc, xml, meta, _bound, error = _raw_call(df, 2, 1)
    assert rc == 3, "YSMR_ERR_CAPACITY"
    assert b"sheet buffer too small" in error
    assert (xml == 0xA5).all() and meta == [-1, -1], "a refused call launches nothing"


# ---- the kinds -----------------------------------------------------------------------------------------------------------------
def device_kinds(data, n_columns):
    from ysmr_amd import _lib
    L = _lib.lib()
    size = len(data)
    text = torch.zeros((size + 255) // 256 * 256, dtype=torch.uint8, device=DEV)
    text[:size] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(DEV)
    ws_bytes = int(L.ysmr_csv_workspace_bytes(size))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    meta = torch.full((4 + _lib.KIND_WORDS,), -1, dtype=torch.int32, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV))
    _lib.check(L.ysmr_csv_index(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, meta.data_ptr(), meta[1:].data_ptr()), "ysmr_csv_index")
    lines, flags = (int(v) & 0xFFFFFFFF for v in meta[:2].cpu())
    _lib.check(L.ysmr_csv_column_kinds(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, n_columns, lines - 1, meta[4:].data_ptr()),
               "ysmr_csv_column_kinds")
    return meta[4:].cpu().numpy().view(np.uint32), lines - 1, flags


def _same_kinds(data, n_columns):
    from ysmr_amd import helper_file as hf
    got, rows, flags = device_kinds(data, n_columns)
    want, want_rows, want_flags = hf.csv_column_kinds_devicelike(data, n_columns)
    assert got.tolist() == want.tolist() and rows == want_rows and flags == want_flags == 0
    assert device_kinds(data, n_columns)[0].tolist() == got.tolist(), "two runs give the same words"
    return got


@pytest.mark.parametrize("name", sorted(xt.kinds_files()))
def test_column_kinds_on_the_device_are_the_twins(name):
    from ysmr_amd import helper_file as hf
    data, n_columns, served = xt.kinds_files()[name]
    assert (hf.column_dtypes_of_kinds(_same_kinds(data, n_columns), n_columns) is not None) == served


@pytest.mark.parametrize("field, bits", (("x", 3), ("", 5), ("12", 1), ("1.25", 1)))
def test_a_deciding_field_beyond_the_staged_span_and_in_the_second_workgroup(field, bits):
    from ysmr_amd import _lib
    chunk, rows_per_group, span = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_csv_geometry(ctypes.byref(chunk), ctypes.byref(rows_per_group), ctypes.byref(span))
    # beyond the span: the line lies further behind its workgroup's first line than LDS holds
    row = rows_per_group.value - 20
    data = xt.long_lines_file(row, rows_per_group.value + 5, field)
    starts = [0] + [k + 1 for k, ch in enumerate(data) if ch == 10]
    assert starts[row + 1] - starts[1] > span.value + 16
    kinds = _same_kinds(data, 16)
    assert kinds[5] == bits and all(int(k) == 1 for c, k in enumerate(kinds[:16]) if c != 5) and kinds[16] == 0
    # the first line of the second workgroup, in a file of short lines
    lines = ["{},{}.5,{}".format(100000 + k, k, -100000 - k) for k in range(rows_per_group.value + 40)]
    parts = lines[rows_per_group.value].split(",")
    parts[2] = field
    lines[rows_per_group.value] = ",".join(parts)
    kinds = _same_kinds(xt._file(lines), 3)
    assert kinds.tolist()[:3] == [0, 1, {"x": 3, "": 5, "12": 0, "1.25": 1}[field]] and kinds[16] == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def results_folder(tmp_path_factory):
    """A result folder as a run leaves it: ``<name>_statistics.csv`` written by ``evaluate_tracks``, an analysed csv with empty
    cells and a csv with a string column (both named so that the collation finds them)."""
    from ysmr_amd import evaluate_tracks, select_tracks
    root = tmp_path_factory.mktemp("xlsx")
    folder = root / "results"
    os.makedirs(folder)
    df = st.make_table(5, n_tracks=25, max_len=500)
    size = df.groupby("TRACK_ID")["TRACK_ID"].transform("size")
    df = df[size >= 32].reset_index(drop=True)
    list_csv = str(root / "clip_list.csv")
    df.to_csv(list_csv, index=False)
    settings = st.select_settings(**{"store processed .csv file": False, "store generated statistical .csv file": True,
                                     "store final analysed .csv file": False, "save large plots": False, "save rose plot": False,
                                     "save angle distribution plot / bins": 0})
    selected = select_tracks(path_to_file=list_csv, results_directory=str(folder), settings=dict(settings), fps=30.0, frame_height=400,
                             frame_width=600)
    assert selected is not None
    assert evaluate_tracks(list_csv, str(folder), df=selected, settings=dict(settings), fps=30.0) is not None
    stats = [f for f in os.listdir(folder) if f.endswith("_statistics.csv")]
    assert len(stats) == 1 and "µm" in open(folder / stats[0], encoding="utf-8").readline()
    analysed = at.analysed(700, seed=3)
    assert analysed["tp_of_tracks"].isna().sum() > 100
    analysed.to_csv(folder / "clip_analysed_statistics.csv", index=False)
    pd.DataFrame({"TRACK_ID": [1, 2, 3], "note": ["a", "b,c", "d"], "v": [0.5, np.nan, 2.0]}).to_csv(folder / "notes_statistics.csv", index=False)
    return str(folder), str(folder / stats[0]).replace(os.sep, "/")


def _book_bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("compress", (False, True))
def test_the_device_paths_workbook_is_the_host_paths(results_folder, tmp_path, compress):
    from ysmr_amd import helper_file as hf
    import xlsx_tools
    folder, stats = results_folder
    os.makedirs(tmp_path / "d")
    on_device = hf.collate_results_csv_to_xlsx(folder, str(tmp_path / "d"), device=DEV, compress=compress)
    taken = dict(hf.LAST_COLLATE)
    assert taken[stats] == "device", "the µ of 'Distance (µm)' does not send a statistics file to the host path"
    assert {os.path.basename(p): v for p, v in taken.items()} == {os.path.basename(stats): "device", "clip_analysed_statistics.csv": "device",
                                                                  "notes_statistics.csv": "host"}
    assert {"file read", "upload", "index + kinds", "parse", "print", "download", "zip"} <= set(hf.LAST_COLLATE_TIMES)
    os.makedirs(tmp_path / "h")
    on_host = hf.collate_results_csv_to_xlsx(folder, str(tmp_path / "h"), device=None, compress=compress)
    assert set(hf.LAST_COLLATE.values()) == {"host"}
    assert _book_bytes(on_device) == _book_bytes(on_host)
    names, sheets, _ = xlsx_tools.read_workbook(on_device)
    assert len(names) == 3 and all(len(sheets[name]) > 10 for name in names)


def test_the_row_cap_on_the_device_path(tmp_path, monkeypatch, caplog):
    from ysmr_amd import helper_file as hf
    monkeypatch.setattr(hf, "XLSX_MAX_ROWS", 5)
    os.makedirs(tmp_path / "in")
    ids = np.arange(9) + 10 ** 13                          # (lines of 14 bytes and more: shorter ones are the host path's)
    pd.DataFrame({"a": ids, "b": np.arange(9) * 0.5}).to_csv(tmp_path / "in" / "long_statistics.csv", index=False)
    # (the kind of column b is decided behind the cap: pandas reads the whole file before it cuts)
    pd.DataFrame({"a": ids, "b": [1, 2, 3, 4, 5, 6, 7, 8.5, np.nan]}).to_csv(tmp_path / "in" / "late_statistics.csv", index=False)
    pd.DataFrame({"a": ids[:5], "b": np.arange(5) * 0.5}).to_csv(tmp_path / "in" / "fits_statistics.csv", index=False)
    books = {}
    for device in (DEV, None):
        os.makedirs(tmp_path / str(device))
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="ysmr"):
            books[device] = _book_bytes(hf.collate_results_csv_to_xlsx(str(tmp_path / "in"), str(tmp_path / str(device)), device=device))
        assert set(hf.LAST_COLLATE.values()) == {"device" if device else "host"}
        warned = [rec.getMessage() for rec in caplog.records if "more than 5 rows" in rec.getMessage()]
        assert len(warned) == 2 and not any("fits_statistics" in w for w in warned)
    assert books[DEV] == books[None]
    assert b'<c r="C6"><v>5.0</v></c>' in books[DEV] and b'r="A6"' in books[DEV] and b'r="A7"' not in books[DEV]


def test_a_file_of_short_lines_is_the_host_paths(tmp_path):
    """The index pass sizes its table of line starts for lines of 14 bytes and more and flags a file with more lines: the
    collation then reads it with pandas -- the same sheet."""
    from ysmr_amd import helper_file as hf
    import xlsx_tools
    os.makedirs(tmp_path / "in")
    pd.DataFrame({"a": np.arange(40), "b": np.arange(40) * 0.5}).to_csv(tmp_path / "in" / "short_statistics.csv", index=False)
    book = hf.collate_results_csv_to_xlsx(str(tmp_path / "in"), str(tmp_path), device=DEV)
    assert list(hf.LAST_COLLATE.values()) == ["host"]
    assert len(xlsx_tools.read_workbook(book)[1]["short_statistics"]) == 2 + 40 * 3
