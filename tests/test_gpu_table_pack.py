"""What the two table printers share behind a staged row (csrc/table_print.h, ``k_table_pack`` of csrc/table_csv.hip), at the
smallest shapes where it changes what it does: ``ysmr_table_format_device`` and ``ysmr_xlsx_sheet_device`` against their host
twins, byte for byte, on ``R + 1`` rows -- two pieces, the second of one row, beginning wherever the first ends -- behind a head
(the csv's header, the sheet's prefix) of every length from 0 to 16 bytes, so that the first piece meets every destination
alignment, the sheet with suffixes of 0, 1 and 17 bytes and its real one; the same with no row at all.  A table of one int8
column has no wide-cell areas, and its csv a second piece of two bytes, shorter than its way to the next 16-byte boundary.
Every call is raw: the output is filled with 0xA5, the capacity is exactly the bound and 256 guard bytes lie behind it, and
nothing at or behind the reported length may change."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch        # before the library is loaded: both then share torch's HIP runtime, as in test_gpu_pipeline.py

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, GUARD = 0xA5, 256
PRINTERS = ("csv", "xlsx")


def rows_per_group(printer):
    from ysmr_amd import _lib
    rows = ctypes.c_int(0)
    if printer == "csv":
        _lib.lib().ysmr_table_format_geometry(ctypes.byref(rows), None)
    else:
        _lib.lib().ysmr_xlsx_sheet_geometry(ctypes.byref(rows), None, None)
    return rows.value


def mixed(n):
    """The five column types; a NaN, a zero and an infinity among the floats and ONE wide cell, in the last row."""
    rng = np.random.default_rng(n + 5)
    f = rng.uniform(-500.0, 500.0, n)
    f[1::7] = np.nan
    f[2::11] = 0.0
    f[3::13] = np.inf
    if n:
        f[-1] = -3.5e-14
    return pd.DataFrame({"u": rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), "l": rng.integers(-2 ** 62, 2 ** 62, n),
                         "i": rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), "b": rng.integers(-128, 128, n).astype(np.int8),
                         "f": f, "g": rng.uniform(0.0, 90.0, n)})


def narrow(n):
    return pd.DataFrame({"b": (np.arange(n) % 10).astype(np.int8)})


def head_of(k):
    return bytes(range(65, 65 + k))


def suffixes(printer):
    from ysmr_amd import helper_file as hf
    return (b"", b">", b"</seventeen bytes>"[:17], hf._SHEET_SUFFIX) if printer == "xlsx" else (None,)


def twin(printer, df, head, suffix):
    from ysmr_amd import helper_file as hf
    if printer == "csv":
        return hf.table_csv_devicelike(df, header=head)
    return hf.xlsx_sheet_devicelike(df, prefix=head, suffix=suffix)


class Raw:
    """The columns of a DataFrame on the device, and raw calls of a printer on them."""

    def __init__(self, printer, df):
        from ysmr_amd import helper_file as hf
        self.printer, self.n = printer, len(df)
        self.dtypes = hf.table_csv_plan(df)[1]
        self.tensors = []
        for k in range(df.shape[1]):
            values = np.ascontiguousarray(df.iloc[:, k].to_numpy())
            self.tensors.append(torch.from_numpy(values.view(np.int32) if values.dtype == np.uint32 else values).to(DEV))
        self.cols = hf._table_columns([t.data_ptr() if self.n else 0 for t in self.tensors], self.dtypes)

    def call(self, head, suffix):
        """-> (the whole output buffer with its guard, reported length, wide cells, bound)"""
        from ysmr_amd import _lib
        L, n, k, cols = _lib.lib(), self.n, len(self.dtypes), self.cols
        if self.printer == "csv":
            bound = int(L.ysmr_table_csv_bound(n, k, cols, len(head)))
            ws_bytes = int(L.ysmr_table_format_workspace_bytes(n, k, cols))
        else:
            bound = int(L.ysmr_xlsx_sheet_bound(n, k, cols, 2, 1, len(head), len(suffix)))
            ws_bytes = int(L.ysmr_xlsx_sheet_workspace_bytes(n, k, cols, 2, 1, len(suffix)))
        assert ws_bytes > 0 and (bound > 0 or not (n or head or suffix))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        out = torch.full((bound + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert out.data_ptr() % 16 == 0, "the head's length is the first piece's alignment"
        meta = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        where = (ws.data_ptr(), ws_bytes, out.data_ptr(), bound, meta.data_ptr(), meta[1:].data_ptr())
        stream = _lib.stream_ptr(torch.device(DEV))
        if self.printer == "csv":
            _lib.check(L.ysmr_table_format_device(stream, n, k, cols, head, len(head), *where), "ysmr_table_format_device")
        else:
            _lib.check(L.ysmr_xlsx_sheet_device(stream, n, k, cols, 2, 1, head, len(head), suffix, len(suffix), *where), "ysmr_xlsx_sheet_device")
        length, wide = meta.tolist()
        return out.cpu().numpy(), length, wide & 0xFFFFFFFF, bound


def check(raw, df, head, suffix):
    expect, expect_wide = twin(raw.printer, df, head, suffix)
    out, length, wide, bound = raw.call(head, suffix)
    what = "{}, head {}, suffix {}".format(raw.printer, len(head), suffix)
    assert length == len(expect) and length <= bound and wide == expect_wide, what
    assert out[:length].tobytes() == expect, what
    assert (out[length:] == FILL).all(), what + ": a byte at or behind the reported length, or in the guard, was written"
    again = raw.call(head, suffix)
    assert again[1] == length and again[0].tobytes() == out.tobytes(), what + ": two calls give the same bytes"
    return expect


@pytest.mark.parametrize("table", ("mixed", "narrow"))
@pytest.mark.parametrize("printer", PRINTERS)
def test_two_pieces_behind_every_head_length(printer, table):
    r = rows_per_group(printer)
    df = {"mixed": mixed, "narrow": narrow}[table](r + 1)
    raw = Raw(printer, df)
    starts = set()
    for k in range(17):
        starts.add(len(twin(printer, df.iloc[:r], head_of(k), b"")[0]) & 15)       # (where the second piece, the last row, begins)
        for suffix in suffixes(printer):
            check(raw, df, head_of(k), suffix)
    assert len(starts) == 16, "the one-row piece began at every alignment"
    if table == "mixed":
        assert twin(printer, df, b"", b"")[1] == 1 and twin(printer, df.iloc[:r], b"", b"")[1] == 0, "one wide cell, in the last row"


@pytest.mark.parametrize("printer", PRINTERS)
def test_no_row_gives_the_head_and_the_suffix_alone(printer):
    df = mixed(0)
    raw = Raw(printer, df)
    for k in (0, 1, 16):
        for suffix in suffixes(printer):
            assert check(raw, df, head_of(k), suffix) == head_of(k) + (suffix or b"")
