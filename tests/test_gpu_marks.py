"""``build_marks_device`` (``ysmr_marks_build``, csrc/marks.hip) against ``annotate.build_marks`` on the table in
``get_data``'s order: the bytes of ``marks`` and of ``first`` are equal, the entries behind the last mark are zero, and a
second run gives the same bytes.  Mark counts around the radix sort's tile of 2048 keys, one, seven and 300 frames, every row
in one frame, frames without marks, a video shorter than the table, tables in track order, shuffled (the rough check sorts
them) and shuffled with an id repeated among the first six (it does not), every subtype."""
import numpy as np
import pandas as pd
import pytest
import torch        # before the library is loaded: both then share torch's HIP runtime, as in test_gpu_table_csv.py

import analysed_tables as at

pytestmark = pytest.mark.gpu

RADIX_TILE = 2048          # csrc/prim.h: keys per workgroup of a radix pass (the library does not report it)


def upload(df):
    """The columns as ``read_typed_device`` leaves them."""
    dev = torch.device("cuda:0")
    ids = df["TRACK_ID"].to_numpy(np.int64)
    assert ((ids >= 0) & (ids < 2 ** 32)).all()
    cols = {"TRACK_ID": ids.astype(np.uint32).view(np.int32), "POSITION_T": df["POSITION_T"].to_numpy(np.int64),
            "POSITION_X": df["POSITION_X"].to_numpy(np.float64), "POSITION_Y": df["POSITION_Y"].to_numpy(np.float64),
            "moving": df["moving"].to_numpy(np.int8), "turn_points": df["turn_points"].to_numpy(np.int8),
            "motility_phenotype": df["motility_phenotype"].to_numpy(np.float64)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cols.items()}


def table_order(df, sort_rule):
    """The table as ``get_data`` hands it on: sorted by (TRACK_ID, POSITION_T) -- always, never, or after the rough check."""
    from ysmr_amd.helper_file import sort_list
    if sort_rule == 1 or (sort_rule == 2 and df.loc[:5, "TRACK_ID"].is_unique):
        return sort_list(df=df.copy())
    return df


def device_marks(columns, n_rows, n_frames, subtype, sort_rule):
    from ysmr_amd.annotate import build_marks_device
    built = build_marks_device(columns, n_rows, n_frames, subtype, sort_rule=sort_rule, device="cuda:0")
    assert built is not None
    torch.cuda.synchronize()
    return built[0].cpu().numpy(), built[1].cpu().numpy()


def check(df, n_frames, subtype=None, sort_rule=2):
    from ysmr_amd.annotate import build_marks
    want, first = build_marks(table_order(df, sort_rule), n_frames, subtype)
    columns = upload(df)
    got, got_first = device_marks(columns, len(df), n_frames, subtype, sort_rule)
    assert got_first.dtype == np.int64 and np.array_equal(got_first, first), (got_first[:8], first[:8])
    m = len(want)
    assert got[:16 * m].tobytes() == want.tobytes(), "marks differ: first at {}".format(
        np.flatnonzero(got[:16 * m].reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[:1] // 16)
    assert len(got) == max(16 * len(df), 16) and not got[16 * m:16 * len(df)].any()
    again, again_first = device_marks(columns, len(df), n_frames, subtype, sort_rule)
    assert again[:16 * len(df)].tobytes() == got[:16 * len(df)].tobytes() and again_first.tobytes() == got_first.tobytes()
    return want, first


@pytest.mark.parametrize("marks", [0, 1, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 6500])
@pytest.mark.parametrize("order", ["track", "shuffled"])
def test_mark_counts_around_the_radix_tile(marks, order):
    """Every row is a mark (no empty cell, every frame inside the video), so the counts are the table's."""
    df = at.analysed(marks, n_frames=300, seed=marks, order=order, nan_share=0.0)
    want, _first = check(df, 300)
    assert len(want) == marks
    if marks == 6500:
        assert df.duplicated(["TRACK_ID", "POSITION_T"]).any()                # the same (id, t) twice: file order decides
        assert want["track_id"].max() >= 4000000000


def test_a_table_whose_rows_are_all_dropped():
    df = at.analysed(700, n_frames=7, seed=1, nan_share=0.0)
    df["POSITION_X"] = np.where(np.arange(700) % 2 == 0, np.nan, np.inf)
    want, first = check(df, 7)
    assert len(want) == 0 and not first.any()


@pytest.mark.parametrize("n_frames", [1, 7, 300])
@pytest.mark.parametrize("order", ["track", "shuffled", "repeat"])
def test_frame_counts_and_table_orders(n_frames, order):
    """The table spans 300 frames: a shorter video drops the rows beyond it.  'shuffled': the rough check sorts; 'repeat': an
    id twice among rows 0 .. 5, so the file's order is the table's."""
    df = at.analysed(3000, n_frames=300, seed=n_frames, order=order)
    assert df["POSITION_T"].max() >= 290 and df.loc[:5, "TRACK_ID"].is_unique == (order == "shuffled")
    want, first = check(df, n_frames)
    assert 0 < len(want) < len(df) and first[-1] == len(want)
    if order != "track" and n_frames == 300:
        by_track, _ = check(df, n_frames, sort_rule=1)
        in_file, _ = check(df, n_frames, sort_rule=0)
        assert by_track.tobytes() != in_file.tobytes()
        assert want.tobytes() == (in_file if order == "repeat" else by_track).tobytes()


def test_every_row_in_one_frame_keeps_the_tables_order():
    df = at.analysed(5000, n_frames=300, seed=11, order="repeat", nan_share=0.0, tracks=60)
    df["POSITION_T"] = np.int64(4)
    want, first = check(df, 7)
    assert len(want) == 5000 and first.tolist() == [0, 0, 0, 0, 0, 5000, 5000, 5000]
    assert np.array_equal(want["track_id"], (df["TRACK_ID"].to_numpy() & 0xFFFFFFFF).astype(np.uint32))     # file order
    df = at.analysed(5000, n_frames=300, seed=12, order="shuffled", nan_share=0.0, tracks=60)
    df["POSITION_T"] = np.int64(0)
    want, first = check(df, 1)                              # 83 rows a track, every (id, t) many times: sorted by id, then file order
    assert len(want) == 5000 and (np.diff(want["track_id"].astype(np.int64)) >= 0).all()


def test_frames_without_marks_and_frames_outside_the_video():
    df = at.analysed(2500, n_frames=300, seed=13, order="shuffled")
    t = df["POSITION_T"].to_numpy().copy()
    t[(t >= 100) & (t < 200)] += 150                        # frames 100 .. 199 hold nothing
    t[::97] = -1 - t[::97]
    t[5::89] = 2 ** 31 + t[5::89]
    t[7::83] = 300                                          # = n_frames
    df["POSITION_T"] = t
    want, first = check(df, 300)
    assert first[100] == first[200] and 0 < first[100] < first[-1] == len(want) < len(df)


@pytest.mark.parametrize("subtype", [0, 1, 2, "motile"])
def test_each_subtype_and_a_nan_phenotype(subtype):
    df = at.analysed(RADIX_TILE + 700, n_frames=40, seed=14, order="shuffled").astype({"motility_phenotype": np.float64})
    df.loc[::5, "motility_phenotype"] = np.nan
    want, _first = check(df, 40, subtype=subtype)
    everything, _ = check(df, 40)
    assert 0 < len(want) < len(everything)


def test_sizes_that_are_refused():
    from ysmr_amd import _lib
    from ysmr_amd.annotate import build_marks_device
    L = _lib.lib()
    assert L.ysmr_marks_workspace_bytes(0, 1) > 0 and L.ysmr_marks_workspace_bytes(1000, 300) >= 24 * 1000
    for n_rows, n_frames in ((-1, 10), (2 ** 31, 10), (10, 0), (10, -1), (10, 2 ** 31 - 1)):
        assert L.ysmr_marks_workspace_bytes(n_rows, n_frames) == 0, (n_rows, n_frames)
    df = at.analysed(10, seed=15)
    assert build_marks_device(upload(df), 10, 0) is None and build_marks_device(upload(df), 10, 2 ** 31) is None
