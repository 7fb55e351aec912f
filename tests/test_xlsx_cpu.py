"""The collated workbook without a GPU: ``collate_results_csv_to_xlsx`` on its host path read back through a reader made of
``zipfile`` and ``xml.etree`` (tests/xlsx_tools.py) and compared with ``pandas.read_csv`` bit for bit; sheet names, the row
cap, ``find_paths`` and the call at the end of ``ysmr()``; the device printer's host twin (``ysmr_xlsx_sheet_devicelike``,
csrc/xlsx_row.h) against ``sheet_xml_host`` byte for byte; and the kinds of a file's columns
(``ysmr_csv_column_kinds_devicelike``) against pandas' dtypes."""
import logging
import os
import struct
import time
import zipfile

import numpy as np
import pandas as pd
import pytest

import xlsx_tables as xt
import xlsx_tools


def _bits(v):
    return struct.pack("<d", float(v))


def _mixed_folder(folder):
    """A folder of files of every sort the host path serves, one in a sub-folder, and one csv the extension leaves out."""
    os.makedirs(os.path.join(folder, "sub"), exist_ok=True)
    rng = np.random.default_rng(3)
    stats = pd.DataFrame({"TRACK_ID": np.arange(5, dtype=np.int64) * 7, "Distance (µm)": rng.uniform(0, 90, 5), "Speed": rng.normal(0, 1e-14, 5),
                          "Turn Points": [0, 1, 2, 3, 4], "empty": [np.nan] * 5, "Arc-Chord Ratio": [0.5, np.nan, -0.0, 1e300, 5e-324]})
    stats.to_csv(os.path.join(folder, "video one_statistics.csv"), index=False)
    mixed = pd.DataFrame({"name": ["a<b", " padded ", "q&\"x\"", None, "ü"], "flag": [True, False, True, True, False],
                          "n": [1, 2, 3, 4, 5], "v": [np.inf, -np.inf, 1.5, np.nan, 2.0 ** -30]})
    mixed.to_csv(os.path.join(folder, "sub", "strings_statistics.csv"), index=False)
    with open(os.path.join(folder, "crlf_statistics.csv"), "wb") as fh:
        fh.write(b"a,b\r\n1,\"x,y\"\r\n2,z\r\n")
    wide = pd.DataFrame({"c{}".format(k): rng.uniform(-5, 5, 4) for k in range(18)})
    wide.to_csv(os.path.join(folder, "eighteen columns_statistics.csv"), index=False)
    with open(os.path.join(folder, "twice_statistics.csv"), "w") as fh:
        fh.write("a,a,b\n1,2,3\n4,5,6\n")
    with open(os.path.join(folder, "not this one.csv"), "w") as fh:
        fh.write("a\n1\n")


def _check_sheet(cells, path):
    """The cells of one sheet against pandas' read of its file."""
    df = pd.read_csv(path, sep=",", header=0, encoding="utf-8")
    by_ref = {ref: (style, kind, text) for ref, style, kind, text in cells}
    assert len(by_ref) == len(cells)
    assert not any(ref == "A1" for ref in by_ref)
    expected = 0
    for k, name in enumerate(df.columns):
        ref = "{}1".format(xlsx_tools.letters(k + 1))
        assert by_ref[ref] == (1, "inlineStr", str(name))
        expected += 1
    for r in range(len(df)):
        assert by_ref["A{}".format(r + 2)] == (1, "n", str(r))
        expected += 1
        for k in range(df.shape[1]):
            ref = "{}{}".format(xlsx_tools.letters(k + 1), r + 2)
            value, dtype = df.iloc[r, k], df.iloc[:, k].dtype
            if dtype == np.int64:
                style, kind, text = by_ref[ref]
                assert (style, kind) == (0, "n") and int(text) == int(value) and text == str(int(value))
            elif dtype == np.float64:
                if np.isnan(value):
                    assert ref not in by_ref, "a NaN cell is absent"
                    continue
                style, kind, text = by_ref[ref]
                if np.isinf(value):
                    assert (style, kind, text) == (0, "inlineStr", "inf" if value > 0 else "-inf")
                else:
                    assert (style, kind) == (0, "n") and _bits(float(text)) == _bits(value), (ref, text, value)
            elif dtype == np.bool_:
                assert by_ref[ref] == (0, "b", "1" if value else "0")
            else:
                if isinstance(value, float) and np.isnan(value):
                    assert ref not in by_ref
                    continue
                assert by_ref[ref] == (0, "inlineStr", str(value))
            expected += 1
    assert expected == len(cells), "no cell beside those of the table"


@pytest.mark.parametrize("compress", (False, True))
def test_the_host_paths_workbook_reads_back_as_pandas_reads_the_files(tmp_path, compress):
    from ysmr_amd import helper_file as hf
    folder = str(tmp_path / "results")
    _mixed_folder(folder)
    paths = hf.find_paths(folder, "statistics.csv")
    assert len(paths) == 5 and not any("not this one" in p for p in paths)
    out = hf.collate_results_csv_to_xlsx(folder, str(tmp_path), device=None, compress=compress)
    assert out is not None and os.path.dirname(out) == str(tmp_path)
    stem = os.path.basename(out)
    assert stem.endswith("_collated_statistics.xlsx") and len(stem) == 12 + len("_collated_statistics.xlsx") and stem[:12].isdigit()
    assert hf.LAST_COLLATE == {p: "host" for p in paths}
    with zipfile.ZipFile(out) as z:
        assert z.testzip() is None
        assert {i.compress_type for i in z.infolist()} == {zipfile.ZIP_DEFLATED if compress else zipfile.ZIP_STORED}
        assert all(i.date_time == (1980, 1, 1, 0, 0, 0) for i in z.infolist())
    names, sheets, members = xlsx_tools.read_workbook(out)
    assert names == hf.xlsx_sheet_names(paths), "sheet order is find_paths' order"
    assert sorted(members) == sorted(["[Content_Types].xml", "_rels/.rels", "xl/workbook.xml", "xl/_rels/workbook.xml.rels", "xl/styles.xml"] +
                                     ["xl/worksheets/sheet{}.xml".format(k + 1) for k in range(5)]), "no shared strings, no docProps"
    for name, path in zip(names, paths):
        _check_sheet(sheets[name], path)
    first = open(out, "rb").read()
    os.remove(out)
    again = hf.collate_results_csv_to_xlsx(folder, str(tmp_path), device=None, compress=compress)
    assert open(again, "rb").read() == first, "the same input files give the same workbook bytes"


def test_no_path_and_no_files(tmp_path, caplog):
    from ysmr_amd import helper_file as hf
    with caplog.at_level(logging.WARNING, logger="ysmr"):
        assert hf.collate_results_csv_to_xlsx(None, str(tmp_path), device=None) is None
        assert any(rec.levelno == logging.CRITICAL for rec in caplog.records)
        caplog.clear()
        assert hf.collate_results_csv_to_xlsx(str(tmp_path), str(tmp_path), device=None) is None
        assert any("Could not find paths." in rec.getMessage() for rec in caplog.records)
    assert os.listdir(tmp_path) == []


def test_a_file_pandas_cannot_read_leaves_no_half_workbook(tmp_path):
    from ysmr_amd import helper_file as hf
    os.makedirs(tmp_path / "in")
    (tmp_path / "in" / "a_statistics.csv").write_text("a,b\n1,2\n")
    (tmp_path / "in" / "b_statistics.csv").write_text("a,b\n1,2\n3,4,5,6\n")
    with pytest.raises(pd.errors.ParserError):
        hf.collate_results_csv_to_xlsx(str(tmp_path / "in"), str(tmp_path), device=None)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".xlsx")]


def test_sheet_names():
    from ysmr_amd import helper_file as hf
    long = "a_video_with_a_long_common_name_"
    assert len(long) == 32
    names = hf.xlsx_sheet_names(["/x/{}{}_statistics.csv".format(long, k) for k in range(3)])
    assert names == [long[:31], long[:29] + "~2", long[:29] + "~3"] and all(len(n) <= 31 for n in names)
    assert hf.xlsx_sheet_names(["/x/a[1]:b*c?d.csv", "q/w\\e.csv"]) == ["a_1__b_c_d", "w_e"]
    assert hf.xlsx_sheet_names(["/x/Video_statistics.csv", "/y/video_STATISTICS.csv", "/z/other.csv"]) == \
        ["Video_statistics", "video_STATISTICS~2", "other"]       # (a short name keeps all of itself in front of the mark)
    many = hf.xlsx_sheet_names(["/x/{}.csv".format("n" * 40)] * 12)
    assert len({n.lower() for n in many}) == 12 and all(len(n) <= 31 for n in many) and many[10] == "n" * 28 + "~11"


def test_the_row_cap_on_the_host_path(tmp_path, monkeypatch, caplog):
    from ysmr_amd import helper_file as hf
    monkeypatch.setattr(hf, "XLSX_MAX_ROWS", 5)
    pd.DataFrame({"a": np.arange(9), "b": np.arange(9) * 0.5}).to_csv(tmp_path / "long_statistics.csv", index=False)
    pd.DataFrame({"a": np.arange(5), "s": list("vwxyz")}).to_csv(tmp_path / "fits_statistics.csv", index=False)
    pd.DataFrame({"a": np.arange(6), "s": list("uvwxyz")}).to_csv(tmp_path / "strings_statistics.csv", index=False)
    with caplog.at_level(logging.WARNING, logger="ysmr"):
        out = hf.collate_results_csv_to_xlsx(str(tmp_path), str(tmp_path), device=None)
    names, sheets, _ = xlsx_tools.read_workbook(out)
    for name in names:
        assert max(xlsx_tools.row_number(ref) for ref, *_ in sheets[name]) == 6
    warned = [rec.getMessage() for rec in caplog.records if "more than 5 rows" in rec.getMessage()]
    assert len(warned) == 2 and any("long_statistics" in w for w in warned) and any("strings_statistics" in w for w in warned)


def test_find_paths(tmp_path, caplog):
    from ysmr_amd import helper_file as hf
    (tmp_path / "deep" / "er").mkdir(parents=True)
    for rel in ("a_statistics.csv", "b_list.csv", "deep/c_statistics.csv", "deep/er/d_statistics.csv"):
        (tmp_path / rel).write_text("x\n1\n")
    base = str(tmp_path)
    assert sorted(hf.find_paths(base, "statistics.csv")) == sorted(base + "/" + rel for rel in ("a_statistics.csv", "deep/c_statistics.csv", "deep/er/d_statistics.csv"))
    assert hf.find_paths(base + "/", "statistics.csv", recursive=False) == [base + "/a_statistics.csv"]
    with caplog.at_level(logging.WARNING, logger="ysmr"):
        assert hf.find_paths(base + "/nowhere", ".csv") is None
    assert any("Path could not be found" in rec.getMessage() for rec in caplog.records)
    old = time.time() - 1000
    os.utime(tmp_path / "b_list.csv", (old, old))
    assert hf.find_paths(base, ".csv", minimal_age=500, recursive=False) == [base + "/b_list.csv"]
    assert hf.find_paths(base, ".csv", maximal_age=500, recursive=False) == [base + "/a_statistics.csv"]
    ahead = time.time() + 1000
    os.utime(tmp_path / "a_statistics.csv", (ahead, ahead))
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="ysmr"):
        assert hf.find_paths(base, ".csv", recursive=False) == [base + "/b_list.csv"]
    assert any("from the future" in rec.getMessage() for rec in caplog.records)
    assert sorted(hf.find_paths(base, ".csv", minimal_age=-1, recursive=False)) == [base + "/a_statistics.csv", base + "/b_list.csv"]
    assert hf.creation_date(base + "/nowhere.csv") is None and hf.creation_date(base + "/b_list.csv") >= 999


def _ysmr_settings(**more):
    from ysmr_amd.helper_file import default_settings
    return default_settings(**dict({"user input": False, "select files": False, "display video analysis": False, "log to file": False}, **more))


def _stub_videos(monkeypatch):
    """The per-video work replaced (as tests/mgpu_stub.py replaces the per-GPU worker): a video leaves its statistics csv.
    The collation is ysmr's own call, made to take the host path: this machine has no GPU."""
    from ysmr_amd import helper_file as hf, main
    calls = []

    def worker(job):
        path, _settings, folder, _device = job[:4]
        name = os.path.splitext(os.path.basename(path))[0]
        pd.DataFrame({"TRACK_ID": [1, 2], "Speed": [0.5, 1.5]}).to_csv(os.path.join(folder, name + "_statistics.csv"), index=False)
        return path, True

    def collate(path, save_path, **kwargs):
        calls.append((path, save_path, dict(kwargs)))
        return hf.collate_results_csv_to_xlsx(path, save_path, **dict(kwargs, device=None))
    monkeypatch.setattr(main, "_worker", worker)
    monkeypatch.setattr(main, "collate_results_csv_to_xlsx", collate)
    return calls


@pytest.mark.parametrize("value, compress", ((True, False), ("Deflate", True), ("yes", False)))
def test_ysmr_ends_with_the_workbook_under_the_two_keys(tmp_path, monkeypatch, value, compress):
    from ysmr_amd import main
    calls = _stub_videos(monkeypatch)
    folder = str(tmp_path / "res")
    done = main.ysmr([str(tmp_path / "v0.avi"), str(tmp_path / "v1.avi")], settings=_ysmr_settings(**{"hip collate xlsx": value}), result_folder=folder)
    assert [r for _, r in done] == [True, True]
    assert calls == [(folder, folder, {"compress": compress})]
    books = [f for f in os.listdir(folder) if f.endswith(".xlsx")]
    assert len(books) == 1
    names, sheets, _ = xlsx_tools.read_workbook(os.path.join(folder, books[0]))
    assert sorted(names) == ["v0_statistics", "v1_statistics"]
    with zipfile.ZipFile(os.path.join(folder, books[0])) as z:
        assert {i.compress_type for i in z.infolist()} == {zipfile.ZIP_DEFLATED if compress else zipfile.ZIP_STORED}


@pytest.mark.parametrize("settings", ({}, {"hip collate xlsx": False}, {"hip collate xlsx": "off"},
                                      {"hip collate xlsx": True, "collate results csv to xlsx": False}))
def test_ysmr_without_the_key_writes_no_workbook(tmp_path, monkeypatch, settings):
    from ysmr_amd import main
    calls = _stub_videos(monkeypatch)
    folder = str(tmp_path / "res")
    main.ysmr([str(tmp_path / "v0.avi")], settings=_ysmr_settings(**settings), result_folder=folder)
    assert calls == [] and not [f for f in os.listdir(folder) if f.endswith(".xlsx")]


def test_a_failing_collation_is_logged_and_swallowed(tmp_path, monkeypatch, caplog):
    from ysmr_amd import main
    _stub_videos(monkeypatch)

    def broken(*_a, **_k):
        raise RuntimeError("no workbook today")
    monkeypatch.setattr(main, "collate_results_csv_to_xlsx", broken)
    with caplog.at_level(logging.ERROR, logger="ysmr"):
        done = main.ysmr([str(tmp_path / "v0.avi")], settings=_ysmr_settings(**{"hip collate xlsx": True}), result_folder=str(tmp_path / "res"))
    assert [r for _, r in done] == [True]
    assert any("no workbook today" in rec.getMessage() for rec in caplog.records)


def test_the_key_is_read_from_the_results_section_of_a_tracking_ini(tmp_path):
    import configparser
    from ysmr_amd import helper_file as hf
    ini = tmp_path / "tracking.ini"

    def write(extra):
        parser = configparser.ConfigParser(allow_no_value=True)
        for section, items in hf.TRACKING_INI.items():
            parser[section] = {k: str(v) for k, v in items}
        parser["RESULTS SETTINGS"].update(extra)
        with open(ini, "w") as fh:
            parser.write(fh)
        return hf.get_configs(str(ini))
    assert "hip collate xlsx" not in write({}) and hf.collate_xlsx_mode(write({})) is None
    assert hf.collate_xlsx_mode(write({"hip collate xlsx": "True"})) == "stored"
    assert hf.collate_xlsx_mode(write({"hip collate xlsx": "DEFLATE"})) == "deflate"
    assert hf.collate_xlsx_mode(write({"hip collate xlsx": "False"})) is None


# ---- the device printer's host twin against the host path ----------------------------------------------------------------------
def _twin(df, first_row, with_index=True):
    from ysmr_amd import helper_file as hf
    text, wide = hf.xlsx_sheet_devicelike(df, first_row=first_row, with_index=with_index, prefix=b"", suffix=b"")
    floats = [c for c in df.columns if df[c].dtype == np.float64]
    assert wide == int(sum(xt.tt.is_wide(df[c]).sum() for c in floats))
    return text


@pytest.mark.parametrize("first_row", (2, 9, 99, 1048570))
@pytest.mark.parametrize("with_index", (True, False))
def test_the_twin_prints_the_five_types_as_the_host_path_does(first_row, with_index):
    df = xt.mixed(7)                                               # (rows 9 -> 10, 99 -> 100; 1048570 + 6: the last legal row)
    assert {df[c].dtype for c in df.columns} == {np.dtype(t) for t in xt.tt.TYPES}
    assert first_row + len(df) - 1 <= xt.LAST_SHEET_ROW
    body = xt.host_body(df, first_row)
    assert _twin(df, first_row, with_index) == (body if with_index else xt.without_index(body))
    assert b"<v>-0.0</v>" in body and b"<v>5e-324</v>" in body and b"<v>1e+300</v>" in body
    assert b"<v>999999999999999999</v>" in body and b"<v>-999999999999999999</v>" in body


def test_the_twin_with_prefix_and_suffix_is_the_whole_sheet():
    from ysmr_amd import helper_file as hf
    df = xt.mixed(40, seed=4)
    assert hf.xlsx_sheet_devicelike(df)[0] == hf.sheet_xml_host(df)
    xlsx_tools.sheet_cells(hf.sheet_xml_host(df))


def test_rows_and_columns_of_only_nan_and_no_rows():
    from ysmr_amd import helper_file as hf
    df = xt.only_floats(6)
    body = xt.host_body(df, 2)
    assert _twin(df, 2) == body
    assert b'<row r="3"><c r="A3" s="1"><v>1</v></c></row>' in body, "a row of only NaN keeps its <row> and its index cell"
    assert b'<c r="C' not in body, "a column of only NaN has no cell"
    assert _twin(df, 2, with_index=False) == xt.without_index(body) and b'<row r="3"></row>' in xt.without_index(body)
    assert _twin(df.iloc[:0], 2) == b""
    assert hf.xlsx_sheet_devicelike(df.iloc[:0])[0] == hf.sheet_xml_host(df.iloc[:0])


def test_sixteen_widest_float_columns_reach_the_plans_longest_row():
    import ctypes
    from ysmr_amd import _lib, helper_file as hf
    rows, staged, longest = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_xlsx_sheet_geometry(ctypes.byref(rows), ctypes.byref(staged), ctypes.byref(longest))
    df = xt.widest_sixteen(7)
    text = _twin(df, 1048570)
    assert text == xt.host_body(df, 1048570)
    cols = hf._table_columns([0] * 16, [np.dtype(np.float64)] * 16)
    L = _lib.lib()
    assert len(text) == L.ysmr_xlsx_sheet_bound(7, 16, cols, 1048570, 1, 0, 0), "every row is as long as the plan's longest row of this table"
    assert len(text) == 7 * (longest.value - 6), "... which the row numbers 0 .. 6, of one digit, keep six bytes below the longest there is"
    assert rows.value * ((longest.value + 3) // 4 * 4) == staged.value <= 65536
    assert L.ysmr_xlsx_sheet_bound(7, 16, cols, 1048570, 1, 10, 5) == len(text) + 15
    assert L.ysmr_xlsx_sheet_bound(1048576, 16, cols, 1, 1, 0, 0) == 1048576 * longest.value
    assert L.ysmr_xlsx_sheet_bound(8, 16, cols, 1048570, 1, 0, 0) == 0, "a row behind the sheet's last is refused"
    assert L.ysmr_xlsx_sheet_bound(1, 16, cols, 0, 1, 0, 0) == 0 and L.ysmr_xlsx_sheet_bound(1, 17, cols, 2, 1, 0, 0) == 0
    assert L.ysmr_xlsx_sheet_workspace_bytes(8, 16, cols, 1048570, 1, 0) == 0


def test_the_twin_refuses_rows_outside_the_sheet_and_a_short_buffer():
    import ctypes
    from ysmr_amd import _lib, helper_file as hf
    L = _lib.lib()
    values = np.arange(3, dtype=np.float64)
    cols = hf._table_columns([values.ctypes.data], [values.dtype])
    out = np.full(4096, 0xA5, np.uint8)
    length, wide = ctypes.c_size_t(0), ctypes.c_longlong(0)
    args = lambda n, first, cap: (n, 1, cols, first, 1, b"", 0, b"", 0, out.ctypes.data, cap, ctypes.byref(length), ctypes.byref(wide))
    assert L.ysmr_xlsx_sheet_devicelike(*args(3, 1048575, 4096)) == _lib.YSMR_ERR_ARG
    bound = L.ysmr_xlsx_sheet_bound(3, 1, cols, 2, 1, 0, 0)
    assert L.ysmr_xlsx_sheet_devicelike(*args(3, 2, bound - 1)) == 3
    assert (out == 0xA5).all()
    assert L.ysmr_xlsx_sheet_devicelike(*args(3, 2, bound)) == 0 and 0 < length.value <= bound


# ---- the kinds of a file's columns -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(xt.kinds_files()))
def test_column_kinds_are_pandas_dtypes_or_a_refusal(name):
    from ysmr_amd import helper_file as hf
    data, n_columns, served = xt.kinds_files()[name]
    kinds, n_rows, flags = hf.csv_column_kinds_devicelike(data, n_columns)
    dtypes = hf.column_dtypes_of_kinds(kinds, n_columns)
    assert flags == 0
    assert (dtypes is not None) == served, (name, [int(k) for k in kinds])
    if dtypes is not None:
        expected, rows = xt.pandas_dtypes(data)
        assert dtypes == expected and n_rows == rows
        assert all(dt in (np.int64, np.float64) for dt in dtypes)
