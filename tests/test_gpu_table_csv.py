"""The device csv writer (csrc/table_csv.hip) on the GPU: ``ysmr_table_format_device`` against the bytes of
``DataFrame.to_csv(index=False)`` -- no tolerance -- at the row counts where its kernels change what they do (a wave, a
workgroup ``R`` of ``ysmr_table_format_geometry``, several workgroups), on the two shapes it is wired to, on rows of all-widest
and all-narrowest fields, with wide cells nowhere, at either end and everywhere; then ``select_tracks`` and ``evaluate_tracks``
with and without 'hip write csv on device' on a small table with stationary tracks."""
import ctypes
import importlib
import os

import numpy as np
import pandas as pd
import pytest
import torch        # before the library is loaded: both then share torch's HIP runtime, as in test_gpu_pipeline.py

import select_tables as st
import table_csv_tables as tt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def geometry():
    from ysmr_amd import _lib
    rows, staged = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_table_format_geometry(ctypes.byref(rows), ctypes.byref(staged))
    return rows.value, staged.value


#: the row counts, R being the rows per workgroup (the library is asked when a test runs: it may not be built at collection)
ROW_COUNTS = ("0", "1", "63", "64", "65", "R - 1", "R", "R + 1", "3 * R + 5")


def upload(df):
    import torch
    tensors = []
    for k in range(df.shape[1]):
        values = np.ascontiguousarray(df.iloc[:, k].to_numpy())
        tensors.append(torch.from_numpy(values.view(np.int32) if values.dtype == np.uint32 else values).to(DEV))
    return tensors


def device_bytes(df, header=None):
    """(text, wide cells) of the device writer for a DataFrame of the five dtypes."""
    import torch
    from ysmr_amd import helper_file
    head, dtypes = helper_file.table_csv_plan(df)
    head = head if header is None else header
    csv, length, wide = helper_file.table_format_device(upload(df), dtypes, len(df), head, torch.device(DEV))
    return csv[:length].cpu().numpy().tobytes(), wide


def wide_count(df):
    return int(sum(tt.is_wide(df[c]).sum() for c in df.columns if df[c].dtype == np.float64))


@pytest.mark.parametrize("count", ROW_COUNTS)
@pytest.mark.parametrize("shape", ("selected", "analysed"))
def test_the_two_shapes_at_the_kernels_row_counts(shape, count):
    n = eval(count, {"R": geometry()[0]})
    df = tt.shaped(tt.SELECTED if shape == "selected" else tt.ANALYSED, n, seed=n + 7)
    got, wide = device_bytes(df)
    assert got == tt.pandas_bytes(df)
    assert wide == wide_count(df)


@pytest.mark.parametrize("wide", ("none", "first", "last", "all"))
def test_wide_cells_nowhere_at_either_end_and_everywhere(wide):
    r = geometry()[0]
    df = tt.shaped(tt.ANALYSED, 3 * r + 5, seed=3, wide=wide)
    expected = {"none": 0, "first": 1, "last": 1, "all": 7 * (3 * r + 5)}[wide]
    assert wide_count(df) == expected
    got, counted = device_bytes(df)
    assert got == tt.pandas_bytes(df)
    assert counted == expected


@pytest.mark.parametrize("rows", ("widest", "narrowest", "alternating"))
def test_rows_of_all_widest_and_all_narrowest_fields(rows):
    r, staged = geometry()
    n = 2 * r + 3                                   # the alternation crosses two workgroup boundaries
    pick = {"widest": lambda k: True, "narrowest": lambda k: False, "alternating": lambda k: k % 2 == 0}[rows]
    for dtypes in ((np.float64,) * 16, tt.TYPES * 3 + (np.int64,)):
        df = tt.uniform_rows(dtypes, n, pick)
        expect = tt.pandas_bytes(df)
        if rows == "widest":
            line = sum(tt.WIDTH[dt] + 1 for dt in dtypes)
            assert len(expect) == len(",".join(df.columns)) + 1 + n * line, "every field is as wide as the bound allows"
            assert r * line <= staged
        got, wide = device_bytes(df)
        assert got == expect
        assert wide == wide_count(df)


@pytest.mark.parametrize("dtype", tt.TYPES)
def test_a_table_of_one_column(dtype):
    r = geometry()[0]
    df = tt.shaped((("only", dtype),), r + 9, seed=11)
    got, wide = device_bytes(df)
    assert got == tt.pandas_bytes(df)
    assert wide == wide_count(df)


def test_sixteen_columns_headers_and_two_runs():
    r = geometry()[0]
    shape = tuple(("k{}".format(k), tt.TYPES[k % 5]) for k in range(16))
    df = tt.shaped(shape, 3 * r + 5, seed=5)
    first, wide = device_bytes(df)
    assert first == tt.pandas_bytes(df) and wide == wide_count(df) and wide > 0
    assert device_bytes(df) == (first, wide), "two runs of one input give the same bytes"
    body = first[first.index(b"\n") + 1:]
    long_header = ("x" * 299 + "\n").encode()
    assert device_bytes(df, header=b"")[0] == body
    assert device_bytes(df, header=long_header)[0] == long_header + body
    assert device_bytes(df.iloc[:0], header=long_header) == (long_header, 0)
    assert device_bytes(df.iloc[:0], header=b"") == (b"", 0)


def test_a_capacity_one_byte_short_is_refused_and_nothing_is_written():
    import torch
    from ysmr_amd import _lib, helper_file
    L = _lib.lib()
    r = geometry()[0]
    df = tt.uniform_rows((np.float64,) * 16, r + 1, lambda k: True)
    head, dtypes = helper_file.table_csv_plan(df)
    tensors = upload(df)
    cols = helper_file._table_columns([t.data_ptr() for t in tensors], dtypes)
    n = len(df)
    bound = int(L.ysmr_table_csv_bound(n, 16, cols, len(head)))
    assert bound == len(tt.pandas_bytes(df))
    ws_bytes = int(L.ysmr_table_format_workspace_bytes(n, 16, cols))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    csv = torch.full((bound + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    meta = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    rc = L.ysmr_table_format_device(_lib.stream_ptr(torch.device(DEV)), n, 16, cols, head, len(head), ws.data_ptr(), ws_bytes,
                                    csv.data_ptr(), bound - 1, meta.data_ptr(), meta[1:].data_ptr())
    assert rc == 3, "YSMR_ERR_CAPACITY"
    assert b"csv buffer too small" in L.ysmr_last_error()
    torch.cuda.synchronize()
    assert bool((csv[bound - 1:] == 0xA5).all()), "nothing behind the capacity"
    assert bool((csv == 0xA5).all()) and meta.tolist() == [-1, -1], "a refused call launches nothing"
    rc = L.ysmr_table_format_device(_lib.stream_ptr(torch.device(DEV)), n, 16, cols, head, len(head), ws.data_ptr(), ws_bytes,
                                    csv.data_ptr(), bound, meta.data_ptr(), meta[1:].data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert csv[:bound].cpu().numpy().tobytes() == tt.pandas_bytes(df) and bool((csv[bound:] == 0xA5).all())


def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def _identical(a, b):
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert list(a.dtypes) == list(b.dtypes) and a.index.equals(b.index)
    for name in a.columns:
        x, y = a[name].to_numpy(), b[name].to_numpy()
        assert x.tobytes() == y.tobytes(), name          # values as bits: -0.0 is not 0.0, a NaN is its payload


def test_select_and_evaluate_write_through_the_device_under_the_key(tmp_path, monkeypatch):
    from ysmr_amd import evaluate_tracks, helper_file, select_tracks
    select_module, evaluate_module = importlib.import_module("ysmr_amd.select"), importlib.import_module("ysmr_amd.evaluate")
    df = st.make_table(5, n_tracks=25, max_len=500)
    size = df.groupby("TRACK_ID")["TRACK_ID"].transform("size")
    df = df[size >= 32].reset_index(drop=True)
    list_csv = str(tmp_path / "clip_list.csv")
    df.to_csv(list_csv, index=False)
    off = st.select_settings(**{"store processed .csv file": True, "store generated statistical .csv file": True,
                                "store final analysed .csv file": True, "save large plots": False, "save rose plot": False,
                                "save angle distribution plot / bins": 0})
    assert "hip write csv on device" not in off
    on = dict(off, **{"hip write csv on device": True})
    taken = []
    real = helper_file.write_table_device

    def spy(frame, save_path, *args, **kwargs):
        path = real(frame, save_path, *args, **kwargs)
        taken.append((os.path.basename(save_path), path, helper_file.LAST_TABLE_WRITE_MARKS.get("wide cells")))
        return path

    def no_pandas_printer(*args, **kwargs):
        raise AssertionError("DataFrame.to_csv was called under the key")
    monkeypatch.setattr(select_module, "write_table_device", spy)
    monkeypatch.setattr(evaluate_module, "write_table_device", spy)
    out = {}
    for name, settings in (("off", off), ("on", on)):
        os.makedirs(tmp_path / name)
        out[name] = select_tracks(path_to_file=list_csv, results_directory=str(tmp_path / name), settings=dict(settings), fps=30.0,
                                  frame_height=400, frame_width=600)
        assert out[name] is not None and len(out[name]) > 100
    assert [t[:2] for t in taken] == [("clip_list_selected_data.csv", "device")]
    _identical(out["on"], out["off"])
    assert _files(tmp_path / "on") == _files(tmp_path / "off") and list(_files(tmp_path / "on")) == ["clip_list_selected_data.csv"]
    # a few of the selected tracks stand still but for rounding noise: steps of a few 2^-44 px
    selected = out["off"].drop(columns="index")
    ids = selected["TRACK_ID"].unique()
    assert len(ids) >= 3
    rng = np.random.default_rng(2)
    for tid in ids[:max(2, len(ids) // 3)]:
        rows = (selected["TRACK_ID"] == tid).to_numpy()
        m = int(rows.sum())
        selected.loc[rows, "POSITION_X"] = 200.25 + rng.integers(-2, 3, m) * 2.0 ** -44
        selected.loc[rows, "POSITION_Y"] = 120.5 + rng.integers(-2, 3, m) * 2.0 ** -44
    selected_csv = str(tmp_path / "still_selected_data.csv")
    selected.to_csv(selected_csv, index=False)
    res = {}
    for name, settings in (("off", off), ("on", on)):
        os.makedirs(tmp_path / ("e" + name))
        if name == "on":
            on_stats = dict(on, **{"store generated statistical .csv file": False})      # (that file stays with pandas)
            with monkeypatch.context() as patch:
                patch.setattr(pd.DataFrame, "to_csv", no_pandas_printer)
                res[name] = evaluate_tracks(selected_csv, str(tmp_path / "eon"), settings=on_stats, fps=30.0)
            os.makedirs(tmp_path / "eon2")
            again = evaluate_tracks(selected_csv, str(tmp_path / "eon2"), settings=dict(on), fps=30.0)
            _identical(again[0], res[name][0])
        else:
            res[name] = evaluate_tracks(selected_csv, str(tmp_path / "eoff"), settings=dict(settings), fps=30.0)
        assert res[name] is not None
    analysed = res["off"][0]
    tiny = tt.is_wide(analysed["travelled_dist"])
    print("travelled_dist: wide cells", int(tiny.sum()), "of", len(analysed), "; tp_of_tracks NaN", int(analysed["tp_of_tracks"].isna().sum()))
    assert tiny.sum() > 20 and analysed["tp_of_tracks"].isna().sum() > 20, "the table must hold what the fast printer declines"
    assert [t[:2] for t in taken[1:]] == [("still_selected_data_analysed.csv", "device")] * 2
    assert taken[1][2] == taken[2][2] == wide_count(analysed) > 0
    _identical(res["on"][0], res["off"][0])
    _identical(res["on"][1], res["off"][1])
    files = _files(tmp_path / "eon2")
    assert files == _files(tmp_path / "eoff")
    assert list(files) == ["still_selected_data_analysed.csv", "still_selected_data_statistics.csv"]
    assert _files(tmp_path / "eon") == {"still_selected_data_analysed.csv": files["still_selected_data_analysed.csv"]}


def test_what_the_writer_does_not_serve_goes_to_pandas(tmp_path):
    from ysmr_amd import helper_file
    base = tt.shaped(tt.SELECTED, 200, seed=9)
    frames = {"float32": base.assign(WIDTH=base["WIDTH"].astype(np.float32)),
              "comma": base.rename(columns={"HEIGHT": "a,b"}),
              "object": base.assign(note="x"),
              "seventeen": pd.DataFrame({"c{}".format(k): np.arange(5, dtype=np.int64) for k in range(17)})}
    for name, frame in frames.items():
        path = str(tmp_path / (name + ".csv"))
        assert helper_file.write_table_device(frame, path, DEV) == "host", name
        assert open(path, "rb").read() == tt.pandas_bytes(frame), name
    # served, with an older file of the name moved aside as save_df_to_csv does, and a non-default index left out as it does
    path = str(tmp_path / "served.csv")
    odd = base.set_index(np.arange(len(base))[::-1])
    assert helper_file.write_table_device(odd, path, DEV) == "device"
    assert helper_file.write_table_device(base.iloc[:50], path, DEV) == "device"
    assert open(path, "rb").read() == tt.pandas_bytes(base.iloc[:50])
    moved = [f for f in os.listdir(tmp_path) if f.endswith(".served.csv")]
    assert len(moved) == 1 and open(tmp_path / moved[0], "rb").read() == tt.pandas_bytes(odd)
    assert helper_file.write_table_device(base.iloc[:7], path, DEV, rename_old_file=False) == "device"
    assert len([f for f in os.listdir(tmp_path) if f.endswith("served.csv")]) == 2
    assert open(path, "rb").read() == tt.pandas_bytes(base.iloc[:7])
