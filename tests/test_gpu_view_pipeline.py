"""'hip save detection video' end to end: ``track_bacteria`` writes ``<name>_detections_output.avi`` during its one pass over
the video, every frame equal to tests/view_model.py's painting of that frame's detections and rows -- taken from a second,
plain ``TrackingPipeline`` run of the same clip --, and leaves the csv and the returned table as they are without the key."""
import functools
import os
import struct

import numpy as np
import pytest

import annotate_model as A
import view_model as V

pytestmark = pytest.mark.gpu

H, W, FRAMES, BATCH = 96, 128, 40, 16          # two full batches and a partial one; the link runs a batch behind


def _settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False,
                            "log to file": False, "minimal frame count": 30, "save video file extension": ".avi",
                            "save video fourcc codec": "DIB "})
    s.update(kw)
    return s


@functools.lru_cache(maxsize=None)
def clip():
    from ysmr_amd.synth import SyntheticVideo
    frames = SyntheticVideo(H, W, 14, seed=33, dropout=0.08, speckle=0.1).frames(FRAMES)
    frames.setflags(write=False)
    return frames


def plain_run(frames, settings, max_det, capacity):
    """Detections and rows of the clip from a TrackingPipeline of its own: (det [n, max_det, 5], det_count [n], rows)."""
    import torch
    from ysmr_amd.track_eval import TrackingPipeline
    pipe = TrackingPipeline(H, W, 30.0, settings, batch=BATCH, max_det=max_det, capacity=capacity)
    dev = torch.from_numpy(np.array(frames)).cuda()
    det, det_count = [], []
    for f0 in range(0, len(frames), BATCH):
        slot, res, ready = pipe.detect_async(dev[f0:f0 + BATCH])
        pipe.link(slot, res, ready, f0)
        torch.cuda.synchronize()
        det.append(res.det.cpu().numpy().copy())
        det_count.append(res.det_count.cpu().numpy().copy())
    pipe.check(res)
    return np.concatenate(det), np.concatenate(det_count), pipe.take_rows()


def run(tmp_path, name, frames, max_det=256, capacity=256, **keys):
    from ysmr_amd.track_eval import track_bacteria
    folder = tmp_path / name
    (folder / "out").mkdir(parents=True)
    path = folder / "clip.npy"
    np.save(path, frames)
    settings = _settings(**keys)
    got = track_bacteria(str(path), settings=settings, result_folder=str(folder / "out"), batch=BATCH, max_det=max_det, capacity=capacity)
    assert got is not None
    return got, str(path), str(folder / "out"), settings


def read_video(path):
    from ysmr_amd.frames import open_video
    video = open_video(path)
    try:
        assert (video.height, video.width, video.channels) == (H, W, 3)
        return video.frame_count, video.read(0, video.frame_count)
    finally:
        video.close()


def same_table(a, b):
    return list(a.columns) == list(b.columns) and all(a[c].to_numpy().tobytes() == b[c].to_numpy().tobytes() for c in a.columns)


MODES = {
    "default": dict(keys={}, max_det=256, capacity=256),
    "per-frame link": dict(keys={}, max_det=1024, capacity=1024),          # capacity above 768: the per-frame kernels emit the rows
    "luminosity": dict(keys={"include luminosity in tracking calculation": True, "disable gsff": True}, max_det=256, capacity=256),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_frame_of_the_file_is_the_models_painting(tmp_path, mode, caplog):
    import logging
    from ysmr_amd import track_eval
    from ysmr_amd.track_eval import detection_video_path
    frames = clip()
    keys, max_det, capacity = MODES[mode]["keys"], MODES[mode]["max_det"], MODES[mode]["capacity"]
    plain, plain_path, plain_out, _ = run(tmp_path, "off", frames, max_det, capacity, **keys)
    assert sorted(os.listdir(plain_out)) == ["clip_list.csv"]                          # with the key off, no file is written
    with caplog.at_level(logging.INFO, logger="ysmr"):
        got, path, out, settings = run(tmp_path, "on", frames, max_det, capacity, **{"hip save detection video": True}, **keys)
    assert track_eval.LAST_PIPELINE_FACTS["batched"] == (mode != "per-frame link")
    written = detection_video_path(path, out, settings)
    assert written == os.path.join(out, "clip_detections_output.avi") and os.path.isfile(written)
    assert written in caplog.text
    assert sorted(os.listdir(out)) == ["clip_detections_output.avi", "clip_list.csv"]
    # the view changes nothing: the csv byte for byte, the table bit for bit, the rest of the result
    assert open(os.path.join(out, "clip_list.csv"), "rb").read() == open(os.path.join(plain_out, "clip_list.csv"), "rb").read()
    assert same_table(got[0], plain[0]) and got[1:4] == plain[1:4]
    count, stored = read_video(written)
    assert count == FRAMES
    det, det_count, rows = plain_run(frames, dict(settings), max_det, capacity)
    assert len(rows) == len(got[0]) and det_count.min() >= 0 and det_count.max() > 5
    assert (rows["disappeared"] > 0).any()                                             # rows of disappeared tracks are painted too
    want = V.paint(frames, det, det_count, rows, 0)
    for i in range(FRAMES):
        assert np.array_equal(stored[i], want[i]), "frame {}: {} pixels differ".format(i, int((stored[i] != want[i]).any(axis=2).sum()))
    base = A.to_bgr(frames)
    assert ((want == (255, 0, 0)).all(axis=3) & (base != want).any(axis=3)).any(axis=(1, 2)).all()      # boxes in every frame
    assert ((want == (0, 255, 0)).all(axis=3) & (base != want).any(axis=3)).any(axis=(1, 2)).all()      # ... and ids


def _payloads(path):
    """The payloads of the '00dc' chunks of an AVI file, in file order."""
    data = open(path, "rb").read()

    def walk(at, end):
        found = []
        while at < end:
            cid, size = struct.unpack_from("<4sI", data, at)
            if cid in (b"RIFF", b"LIST"):
                found += walk(at + 12, at + 8 + size)
            elif cid == b"00dc":
                found.append(data[at + 8:at + 8 + size])
            at += 8 + size + (size & 1)
        return found

    return walk(0, len(data))


def test_motion_jpeg_chunks_are_the_models_encoding_of_the_uncompressed_frames(tmp_path):
    import jpeg_model as jm
    from ysmr_amd.track_eval import detection_video_path
    frames = clip()
    raw, raw_path, raw_out, s = run(tmp_path, "raw", frames, **{"hip save detection video": True})
    _, stored = read_video(detection_video_path(raw_path, raw_out, s))
    got, path, out, s = run(tmp_path, "mjpg", frames, **{"hip save detection video": True, "save video fourcc codec": "MJPG",
                                                           "hip video jpeg quality": 85})
    payloads = _payloads(detection_video_path(path, out, s))
    assert len(payloads) == FRAMES
    for i in range(FRAMES):
        assert payloads[i] == jm.encode(stored[i], 85), "frame {}".format(i)
    assert same_table(got[0], raw[0])
    assert open(os.path.join(out, "clip_list.csv"), "rb").read() == open(os.path.join(raw_out, "clip_list.csv"), "rb").read()


def test_an_overflow_rerun_starts_the_file_over(tmp_path, caplog):
    from ysmr_amd.track_eval import detection_video_path
    frames = clip()
    plain, _, _, _ = run(tmp_path, "roomy", frames, **{"hip save detection video": True})
    # eight detections per frame are too few: the pass is repeated with doubled buffers until the clip fits
    got, path, out, s = run(tmp_path, "tight", frames, max_det=8, capacity=8, **{"hip save detection video": True})
    assert "running it again" in caplog.text
    count, stored = read_video(detection_video_path(path, out, s))
    _, roomy = read_video(os.path.join(str(tmp_path / "roomy" / "out"), "clip_detections_output.avi"))
    assert count == FRAMES and np.array_equal(stored, roomy) and same_table(got[0], plain[0])


def test_a_failed_pass_removes_the_partial_file_and_bad_settings_write_none(tmp_path, caplog, monkeypatch):
    from ysmr_amd import _lib, track_eval
    frames = clip()
    folder = tmp_path / "fails"
    (folder / "out").mkdir(parents=True)
    np.save(folder / "clip.npy", frames)
    target = os.path.join(str(folder / "out"), "clip_detections_output.avi")
    seen = []

    def check(self, res):      # the pipeline's look at its error flags, behind the first linked batch
        seen.append(os.path.isfile(target))
        raise _lib.YsmrLibraryError("made to fail")

    monkeypatch.setattr(track_eval.TrackingPipeline, "check", check)
    s = _settings(**{"hip save detection video": True})
    assert track_eval.track_bacteria(str(folder / "clip.npy"), settings=s, result_folder=str(folder / "out"), batch=BATCH,
                                     max_det=256, capacity=256) is None
    assert seen == [True] and "made to fail" in caplog.text
    assert not os.path.exists(target)
    monkeypatch.undo()
    s = _settings(**{"hip save detection video": True, "save video fourcc codec": "MJPG", "hip video jpeg quality": 0})
    assert track_eval.track_bacteria(str(folder / "clip.npy"), settings=s, result_folder=str(folder / "out"), batch=BATCH,
                                     max_det=256, capacity=256) is None
    assert "hip video jpeg quality" in caplog.text and not os.path.exists(target)


def test_a_file_that_cannot_be_opened_ends_the_view_and_tracking_goes_on(tmp_path, caplog):
    frames = clip()
    plain, _, _, _ = run(tmp_path, "plain", frames)
    folder = tmp_path / "blocked"
    (folder / "out" / "clip_detections_output.avi").mkdir(parents=True)          # a directory where the file is to go
    np.save(folder / "clip.npy", frames)
    from ysmr_amd.track_eval import track_bacteria
    for codec in ("DIB ", "MJPG"):
        s = _settings(**{"hip save detection video": True, "save video fourcc codec": codec})
        got = track_bacteria(str(folder / "clip.npy"), settings=s, result_folder=str(folder / "out"), batch=BATCH, max_det=256, capacity=256)
        assert got is not None and same_table(got[0], plain[0])
    assert caplog.text.count("is not written") == 2
    assert os.path.isdir(str(folder / "out" / "clip_detections_output.avi"))


@pytest.mark.skipif(__import__("torch").cuda.device_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("codec", ["DIB ", "MJPG"])
def test_the_view_on_the_second_gpu_while_the_first_is_current(tmp_path, codec):
    """Every launch of the view goes to the device its buffers live on, whatever the caller's current device is (a fresh
    worker's is cuda:0): the same file and the same table as on cuda:0."""
    import torch
    from ysmr_amd.track_eval import detection_video_path, track_bacteria
    frames = clip()
    keys = {"hip save detection video": True, "save video fourcc codec": codec, "hip video jpeg quality": 85}
    first, path, out, s = run(tmp_path, "first", frames, **keys)
    folder = tmp_path / "second"
    (folder / "out").mkdir(parents=True)
    np.save(folder / "clip.npy", frames)
    torch.cuda.set_device(0)
    got = track_bacteria(str(folder / "clip.npy"), settings=_settings(**keys), result_folder=str(folder / "out"), batch=BATCH,
                         max_det=256, capacity=256, device="cuda:1")
    assert got is not None and torch.cuda.current_device() == 0 and same_table(got[0], first[0])
    written = detection_video_path(str(folder / "clip.npy"), str(folder / "out"), s)
    assert open(written, "rb").read() == open(detection_video_path(path, out, s), "rb").read()


def test_annotate_video_writes_what_it_wrote_before_its_output_path_was_shared(tmp_path):
    """annotate_video goes through the same DibOutput as the view: its file against annotate_model, uncompressed and
    Motion-JPEG, in batches of 16, 16 and 8 frames."""
    import jpeg_model as jm
    import pandas as pd
    from ysmr_amd import annotate_video
    frames = clip()
    rng = np.random.default_rng(9)
    table, per_frame = [], [[] for _ in range(FRAMES)]
    for track in (2, 31, 456, 70000):
        x, y = float(rng.integers(10, W - 10)), float(rng.integers(20, H - 5))
        for t in range(int(rng.integers(0, 5)), FRAMES - int(rng.integers(0, 5))):
            x, y = x + rng.uniform(-2, 2), y + rng.uniform(-2, 2)
            moving, turn = int(rng.random() < 0.7), int(rng.random() < 0.3)
            table.append((track, t, x, y, moving, turn, 2))
            per_frame[t].append((int(x), int(y), track, 1 if moving == 0 else 2 if turn == 1 else 0))
    df = pd.DataFrame(table, columns=["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "moving", "turn_points", "motility_phenotype"])
    df = df.astype({"TRACK_ID": np.int64, "POSITION_T": np.int64, "moving": np.int8, "turn_points": np.int8, "motility_phenotype": np.int8})
    marks = np.array([m for f in per_frame for m in f], dtype=A.MARK_DTYPE)
    first = np.concatenate([[0], np.cumsum([len(f) for f in per_frame])]).astype(np.int64)
    want = A.paint(frames, marks, first)
    path = str(tmp_path / "clip.npy")
    np.save(path, frames)
    s = _settings(**{"hip frames per batch": BATCH})
    written = annotate_video(path, df, settings=s, result_folder=str(tmp_path / "raw"))
    assert written is not None
    count, stored = read_video(written)
    assert count == FRAMES and np.array_equal(stored, want)
    s = _settings(**{"hip frames per batch": BATCH, "save video fourcc codec": "MJPG", "hip video jpeg quality": 85})
    written = annotate_video(path, df, settings=s, result_folder=str(tmp_path / "mjpg"))
    assert written is not None
    assert _payloads(written) == [jm.encode(f, 85) for f in want]
