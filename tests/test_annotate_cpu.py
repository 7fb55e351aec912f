"""The annotated output video without a GPU: the C ABI's new entry point, the AVI writer, the marks built from an
evaluated table, and the wiring in ``analyse``."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import annotate_model as am
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from ysmr_amd import _lib
    return _lib.lib()


def test_annotate_batch_is_declared_exported_and_bound(lib):
    from ysmr_amd import _lib
    header = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    decl = re.search(r"int\s+ysmr_annotate_batch\s*\(([^;]*)\)\s*;", header)
    assert decl, "ysmr_annotate_batch is not declared in include/ysmr_hip.h"
    args = " ".join(decl.group(1).split())
    assert args == ("void *stream, const uint8_t *frames_dev, int n_frames, int height, int width, int channels, "
                    "const ysmr_mark *marks_dev, const int64_t *first_dev, "
                    "uint8_t *out_dev, int out_stride, size_t out_frame_bytes, int bottom_up")
    assert re.search(r"int32_t\s+x,\s*y;\s*uint32_t\s+track_id;\s*uint32_t\s+style;\s*}\s*ysmr_mark;", header)
    assert "ysmr_annotate_batch" in _lib.EXPORTS and hasattr(lib, "ysmr_annotate_batch")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib.ysmr_annotate_batch.argtypes == [vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, ctypes.c_size_t, ci]
    assert lib.ysmr_annotate_batch.restype is ci
    assert _lib.MARK_DTYPE == am.MARK_DTYPE and _lib.MARK_DTYPE.itemsize == 16
    assert int(re.search(r"#define YSMR_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 15


def test_annotate_batch_rejects_bad_arguments(lib):
    from ysmr_amd import _lib
    some = ctypes.c_void_p(4096)         # never dereferenced: every call below fails its argument checks
    assert lib.ysmr_annotate_batch(None, None, 1, 4, 4, 1, None, None, some, 12, 48, 1) == _lib.YSMR_ERR_ARG
    assert b"NULL" in lib.ysmr_last_error()
    assert lib.ysmr_annotate_batch(None, some, 1, 4, 4, 1, None, None, None, 12, 48, 1) == _lib.YSMR_ERR_ARG
    assert lib.ysmr_annotate_batch(None, some, 1, 4, 4, 2, None, None, some, 12, 48, 1) == _lib.YSMR_ERR_ARG
    assert b"channels" in lib.ysmr_last_error()
    assert lib.ysmr_annotate_batch(None, some, 1, 4, 4, 1, None, None, some, 8, 48, 1) == _lib.YSMR_ERR_ARG     # stride < 3 W
    assert b"out_stride" in lib.ysmr_last_error()
    assert lib.ysmr_annotate_batch(None, some, 1, 4, 4, 1, None, None, some, 12, 44, 1) == _lib.YSMR_ERR_ARG    # frame < 4 rows
    assert lib.ysmr_annotate_batch(None, some, 0, 4, 4, 1, None, None, some, 12, 48, 1) == _lib.YSMR_ERR_ARG
    assert lib.ysmr_annotate_batch(None, some, 1, 4, 4, 1, None, some, some, 12, 48, 1) == _lib.YSMR_ERR_ARG    # first without marks


# ---- the writer ------------------------------------------------------------------------------------------------------

def _frames(n=7, h=9, w=13, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("bottom_up", [True, False])
def test_writer_round_trip_is_exact(tmp_path, bottom_up):
    from ysmr_amd.annotate import AviWriter
    from ysmr_amd.frames import AviVideo
    frames = _frames()
    path = str(tmp_path / "a.avi")
    w = AviWriter(path, 13, 9, 30000 / 1001, bottom_up=bottom_up)
    assert (w.stride, w.frame_bytes, w.rate, w.scale) == (40, 360, 30000, 1001)
    w.write(am.pack_dib(frames, bottom_up))
    w.close()
    v = AviVideo(path)
    assert (v.frame_count, v.frames_available, v.height, v.width, v.channels) == (7, 7, 9, 13, 3)
    assert v.fps == 30000 / 1001
    assert np.array_equal(v.read(0, 7), frames)
    v.close()
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"AVI " and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8
    assert raw.count(b"AVIX") == 0 and raw.count(b"00db") == 7 + 7          # seven chunks, seven idx1 entries
    avih = raw.index(b"avih") + 8
    usec, _, _, flags, total, _, streams, _, width, height = struct.unpack("<10I", raw[avih:avih + 40])
    assert (usec, flags & 0x10, total, streams, width, height) == (33367, 0x10, 7, 1, 13, 9)
    strf = raw.index(b"strf") + 8
    size, bw, bh, planes, bits, compression, image = struct.unpack("<IiiHHII", raw[strf:strf + 24])
    assert (size, bw, bh, planes, bits, compression, image) == (40, 13, 9 if bottom_up else -9, 1, 24, 0, 360)
    idx = raw.index(b"idx1")
    movi = raw.index(b"movi")
    assert struct.unpack("<I", raw[idx + 4:idx + 8])[0] == 16 * 7 and idx + 8 + 16 * 7 == len(raw)
    for k in range(7):
        cid, kf, off, sz = struct.unpack("<4sIII", raw[idx + 8 + 16 * k:idx + 24 + 16 * k])
        assert (cid, kf, sz) == (b"00db", 0x10, 360) and raw[movi + off:movi + off + 4] == b"00db"


def test_writer_continues_in_avix_segments(tmp_path):
    """riff_limit of a few kilobytes: three segments, every one within the limit, read back exactly; frames with and
    without their chunk headers in front go to the same file."""
    from ysmr_amd.annotate import AviWriter
    from ysmr_amd.frames import AviVideo
    frames = _frames(n=8)
    path = str(tmp_path / "a.avi")
    w = AviWriter(path, 13, 9, 25, riff_limit=1300)
    dib = am.pack_dib(frames, True)
    w.write(dib[:1])
    chunks = np.zeros((7, w.frame_bytes + 8), np.uint8)
    chunks[:, :8] = np.frombuffer(w.chunk_header(), np.uint8)
    chunks[:, 8:] = dib[1:]
    w.write_chunks(chunks)
    w.close()
    raw = open(path, "rb").read()
    # first segment: 248 header bytes + 2 x (368 + 16) + 8 = 1024 (a third frame would make 1408); then 3 x 368 + 24 = 1128
    starts = [m.start() for m in re.finditer(b"RIFF", raw)]
    assert len(starts) == 3 and raw.count(b"AVIX") == 2
    sizes = [struct.unpack("<I", raw[s + 4:s + 8])[0] + 8 for s in starts]
    assert sizes == [1024, 1128, 1128] and sum(sizes) == len(raw) and all(s <= 1300 for s in sizes)
    v = AviVideo(path)
    assert (v.frame_count, v.frames_available, v.fps) == (8, 8, 25.0)
    assert np.array_equal(v.read(0, 8), frames)
    v.close()
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / "b.avi"), 13, 9, 25).write_chunks(np.zeros((2, 360), np.uint8))


def test_writer_abort_removes_the_file(tmp_path):
    from ysmr_amd.annotate import AviWriter
    path = str(tmp_path / "a.avi")
    w = AviWriter(path, 13, 9, 25)
    w.write(am.pack_dib(_frames(n=1), True))
    w.abort()
    assert not os.path.exists(path)
    assert AviWriter.file_bytes(13, 9, 7) >= 248 + 7 * (368 + 16) + 8


# ---- the marks -------------------------------------------------------------------------------------------------------

def _table():
    import pandas as pd
    rows = [  # TRACK_ID, POSITION_T, X, Y, moving, turn_points, motility_phenotype
        (7, 2, 10.9, 20.2, 1, 0, 2),            # 0  green
        (7, 0, 11.9, -0.9, 1, 1, 2),            # 1  white; -0.9 truncates to 0, not -1
        (3, 2, -5.7, 8.5, 0, 1, 0),             # 2  orange (not moving wins over the turn point); -5.7 -> -5
        (3, 1, np.nan, 3.0, 1, 0, 0),           # 3  not finite: skipped
        (9, 2, 1.0, 2.0, 1, 0, 1),              # 4  frame 2 again: after rows 0 and 2
        (9, 5, 1.0, 2.0, 1, 0, 1),              # 5  frame 5 of a 5-frame video: skipped
        (4294967295, 4, 3e12, np.inf, 1, 0, 2),  # 6  not finite
        (4294967295, 4, 3.0, 4.99, 1, 1, 2),    # 7  white
    ]
    cols = ["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "moving", "turn_points", "motility_phenotype"]
    df = pd.DataFrame(rows, columns=cols)
    return df.astype({"TRACK_ID": np.int64, "POSITION_T": np.int64, "moving": np.int8, "turn_points": np.int8,
                      "motility_phenotype": np.int8})


def test_marks_from_a_table():
    from ysmr_amd.annotate import build_marks
    marks, first = build_marks(_table(), 5)
    assert marks.dtype == am.MARK_DTYPE and first.dtype == np.int64
    assert first.tolist() == [0, 1, 1, 4, 4, 5]
    assert [tuple(int(v) for v in m) for m in marks] == [
        (11, 0, 7, 2), (10, 20, 7, 0), (-5, 8, 3, 1), (1, 2, 9, 0), (3, 4, 4294967295, 2)]
    # the subtype filter: by code or by name, the same rows
    for which in (2, "motile"):
        marks, first = build_marks(_table(), 5, select_subtype=which)
        assert first.tolist() == [0, 1, 1, 2, 2, 3] and marks["track_id"].tolist() == [7, 7, 4294967295]
    marks, first = build_marks(_table(), 5, select_subtype="immotile")
    assert first.tolist() == [0, 0, 0, 1, 1, 1] and marks["x"].tolist() == [-5]
    marks, first = build_marks(_table().assign(motility_phenotype=lambda d: d["motility_phenotype"].astype(str).astype(object)),
                               5, select_subtype=1)          # the column as a csv read with upstream's dtypes delivers it
    assert marks["track_id"].tolist() == [9]
    marks, first = build_marks(_table().iloc[:0], 3)
    assert len(marks) == 0 and first.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        build_marks(_table(), 5, select_subtype="swimming")


def test_annotate_video_refusals_without_a_gpu(tmp_path, caplog):
    from ysmr_amd import annotate_video, track_eval
    from ysmr_amd.annotate import annotate_video as direct
    from ysmr_amd.helper_file import default_settings
    assert annotate_video is direct and track_eval.annotate_video is direct
    s = default_settings(**{"log to file": False})
    np.save(tmp_path / "clip.npy", np.zeros((3, 8, 8), np.uint8))
    assert direct(str(tmp_path / "clip.npy"), _table(), output_save=False, settings=s, result_folder=str(tmp_path)) is None
    assert "interactive display" in caplog.text
    assert direct(str(tmp_path / "missing.npy"), _table(), settings=s, result_folder=str(tmp_path)) is None
    assert "Cannot open file" in caplog.text
    assert not [n for n in os.listdir(tmp_path) if n.endswith(".avi")]


# ---- the wiring ------------------------------------------------------------------------------------------------------

def test_analyse_hands_evaluates_table_to_annotate_video(tmp_path, monkeypatch, caplog):
    from ysmr_amd import main
    from ysmr_amd.helper_file import default_settings
    table, stats, calls = _table(), object(), []
    monkeypatch.setattr(main, "track_bacteria", lambda **kw: ("tracked", 30.0, 8, 8, None))
    monkeypatch.setattr(main, "select_tracks", lambda **kw: "selected")
    monkeypatch.setattr(main, "evaluate_tracks", lambda **kw: (table, stats))
    monkeypatch.setattr(main, "annotate_video", lambda **kw: calls.append(kw))
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                            "save video": True})
    video = str(tmp_path / "clip.npy")
    out = str(tmp_path / "out")
    assert main.analyse(video, settings=s, result_folder=out, device="cuda:3") is True
    assert len(calls) == 1 and calls[0]["df"] is table
    assert {k: v for k, v in calls[0].items() if k != "df"} == {"video_path": video, "settings": s, "result_folder": out,
                                                                 "device": "cuda:3"}
    # evaluate_tracks failed: nothing to annotate
    monkeypatch.setattr(main, "evaluate_tracks", lambda **kw: None)
    assert main.analyse(video, settings=s, result_folder=out) is None and len(calls) == 1
    # a table of an earlier run: upstream's warning, no call
    monkeypatch.setattr(main, "evaluate_tracks", lambda **kw: (table, stats))
    assert main.analyse(str(tmp_path / "clip_list.csv"), settings=s, result_folder=out) is True
    assert len(calls) == 1
    assert "'save video' setting is enabled but .csv file was provided" in caplog.text
    # 'save video' off (the default): as before
    caplog.clear()
    assert main.analyse(video, settings=dict(s, **{"save video": False}), result_folder=out) is True
    assert len(calls) == 1 and "save video" not in caplog.text
