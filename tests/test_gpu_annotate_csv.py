"""``annotate_video`` handed the path of an ``*_analysed.csv``: under 'hip read csv on device' the table is read
(``read_typed_device``) and its marks are built (``build_marks_device``) on the GPU, and the written file has the bytes the
pandas + ``build_marks`` path writes, uncompressed and as Motion-JPEG; a csv the device reader does not serve gives the same
file again, through the host path.  ``LAST_MARKS`` says which way a call went."""
import os

import numpy as np
import pytest
import torch        # before the library is loaded: both then share torch's HIP runtime, as in test_gpu_table_csv.py

import analysed_tables as at

pytestmark = pytest.mark.gpu

KEY = "hip read csv on device"
N_FRAMES, HEIGHT, WIDTH = 12, 48, 64


def clip_and_table(tmp_path, order):
    """A 12-frame 48 x 64 gray clip and a table of 900 rows over 14 frames (two beyond the clip), positions inside and a little
    outside the frame, some cells empty."""
    rng = np.random.default_rng(5)
    clip = str(tmp_path / "clip.npy")
    np.save(clip, rng.integers(0, 200, (N_FRAMES, HEIGHT, WIDTH), dtype=np.uint8))
    df = at.analysed(900, n_frames=N_FRAMES + 2, seed=21, order=order, tracks=30)
    df["POSITION_X"] = df["POSITION_X"] * (WIDTH + 10) / 2020.0
    df["POSITION_Y"] = df["POSITION_Y"] * (HEIGHT + 10) / 1120.0
    csv = str(tmp_path / "clip_analysed.csv")
    df.to_csv(csv, index=False)
    return clip, csv, df


def settings(codec, **more):
    from ysmr_amd.helper_file import default_settings
    return default_settings(**{"log to file": False, "hip frames per batch": 5, "frames per second": 25.0,
                               "save video file extension": ".avi", "save video fourcc codec": codec, **more})


def run(clip, csv, folder, s, **kwargs):
    from ysmr_amd import annotate, annotate_video
    written = annotate_video(clip, csv, settings=s, result_folder=str(folder), **kwargs)
    assert written is not None and os.path.isfile(written)
    with open(written, "rb") as fh:
        return fh.read(), dict(annotate.LAST_MARKS)


@pytest.mark.parametrize("codec", ["DIB ", "MJPG"])
@pytest.mark.parametrize("order", ["track", "shuffled"])
def test_the_file_is_the_same_with_and_without_the_key(tmp_path, codec, order):
    clip, csv, df = clip_and_table(tmp_path, order)
    off = settings(codec)
    assert KEY not in off
    host, went_host = run(clip, csv, tmp_path / "host", off)
    device, went_device = run(clip, csv, tmp_path / "device", dict(off, **{KEY: True}))
    want, _first = at.reference_marks(csv, N_FRAMES)
    assert went_host == {"path": "host", "rows": len(df), "marks": len(want)} and 0 < len(want) < len(df)
    assert went_device == {"path": "device", "rows": len(df), "marks": len(want)}
    assert device == host, "{} of {} bytes differ".format(
        int((np.frombuffer(device, np.uint8)[:len(host)] != np.frombuffer(host, np.uint8)[:len(device)]).sum()), len(host))
    # the marks did something: the file without them is another
    empty = str(tmp_path / "empty_analysed.csv")
    df.iloc[:0].to_csv(empty, index=False)
    bare, went_empty = run(clip, empty, tmp_path / "bare", dict(off, **{KEY: True}))
    assert went_empty == {"path": "device", "rows": 0, "marks": 0} and bare != host and len(bare) > 0


def test_a_subtype_is_selected_on_the_device_too(tmp_path):
    clip, csv, df = clip_and_table(tmp_path, "shuffled")
    off = settings("DIB ")
    host, went_host = run(clip, csv, tmp_path / "host", off, select_subtype="motile")
    device, went_device = run(clip, csv, tmp_path / "device", dict(off, **{KEY: True}), select_subtype="motile")
    everything, _ = run(clip, csv, tmp_path / "all", off)
    assert went_host["path"] == "host" and went_device["path"] == "device" and 0 < went_device["marks"] == went_host["marks"]
    assert device == host and host != everything


def test_a_data_frame_argument_and_an_unserved_csv_go_the_host_way(tmp_path):
    from ysmr_amd import annotate
    from ysmr_amd.helper_file import get_data
    clip, csv, df = clip_and_table(tmp_path, "track")
    on = settings("DIB ", **{KEY: True})
    served, went = run(clip, csv, tmp_path / "served", on)
    assert went["path"] == "device"
    # a nan literal: pandas reads it as the empty cell, the device reader does not serve it
    lines = open(csv).read().split("\n")
    row = next(k for k in range(1, len(lines)) if lines[k].split(",")[2] == "")
    cells = lines[row].split(",")
    cells[2] = "nan"
    unserved = str(tmp_path / "other" / "clip_analysed.csv")
    os.makedirs(os.path.dirname(unserved))
    with open(unserved, "w") as fh:
        fh.write("\n".join(lines[:row] + [",".join(cells)] + lines[row + 1:]))
    same, went = run(clip, unserved, tmp_path / "unserved", on)
    assert went["path"] == "host" and same == served
    frame, went = run(clip, get_data(csv, dtype=at.PANDAS_DTYPE), tmp_path / "frame", on)
    assert went["path"] == "frame" and frame == served
    # a csv that nobody can read is None, as without the key
    from ysmr_amd import annotate_video
    assert annotate_video(clip, str(tmp_path / "missing_analysed.csv"), settings=on, result_folder=str(tmp_path / "none")) is None
    assert annotate_video(clip, str(tmp_path / "missing_analysed.csv"), settings=settings("DIB "), result_folder=str(tmp_path / "none")) is None
    assert annotate.LAST_MARKS == {}
