"""'hip save threshold video' end to end: ``track_bacteria`` writes ``<name>_threshold_output.avi`` during its one pass over the
video, every frame equal to tests/thrview_model.py's painting of the maps that oracle/ysmr_oracle.py computes for that frame
on the CPU -- the class map and the mask behind the hysteresis --, and leaves the csv and the returned table as they are
without the key.  The clip (tests/thrview_clips.py) is 13 frames in batches of 4: the last batch holds one frame."""
import logging
import os

import numpy as np
import pytest

import thrview_clips as C
import thrview_model as T
from test_gpu_view_pipeline import _payloads, same_table

pytestmark = pytest.mark.gpu

NAME = "clip_threshold_output.avi"


def _settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                            "minimal frame count": 10, "save video file extension": ".avi", "save video fourcc codec": "DIB "})
    s.update(kw)
    return s


def run(tmp_path, name, frames, max_det=256, capacity=256, expect=True, **keys):
    from ysmr_amd.track_eval import track_bacteria
    folder = tmp_path / name
    (folder / "out").mkdir(parents=True)
    path = folder / "clip.npy"
    np.save(path, frames)
    settings = _settings(**keys)
    got = track_bacteria(str(path), settings=settings, result_folder=str(folder / "out"), batch=C.BATCH, max_det=max_det, capacity=capacity)
    assert (got is not None) == expect
    return got, str(path), str(folder / "out"), settings


def read_video(path):
    from ysmr_amd.frames import open_video
    video = open_video(path)
    try:
        assert (video.height, video.width, video.channels) == (C.H, C.W, 3)
        return video.frame_count, video.read(0, video.frame_count)
    finally:
        video.close()


def csv_of(out):
    return open(os.path.join(out, "clip_list.csv"), "rb").read()


def assert_frames(stored, want):
    assert len(stored) == len(want) == C.FRAMES
    for i in range(C.FRAMES):
        assert np.array_equal(stored[i], want[i]), "frame {}: {} pixels differ".format(i, int((stored[i] != want[i]).any(axis=2).sum()))


@pytest.mark.parametrize("kind", ["gray", "bgr"])
def test_the_oracles_maps_hold_all_three_classes(kind):
    """What the 'classes' runs below rest on, from the CPU oracle alone: kept markers, kept pixels that are no markers and
    pixels dropped by the hysteresis, all three in one frame (here: in every frame), and visible in the expected picture."""
    counts = C.classes_per_frame(kind)
    assert (counts > 0).all(axis=1).any(), counts.tolist()
    want = C.expected(kind, "classes")
    for colour in (T.KEPT_MARKER, T.KEPT, T.DROPPED):
        assert (want == colour).all(axis=3).any(axis=(1, 2)).all(), colour
    assert (C.expected(kind, "markers") != C.expected(kind, "mask")).any()


@pytest.mark.parametrize("kind", ["gray", "bgr"])
@pytest.mark.parametrize("mode", ["mask", "markers", "classes"])
def test_every_frame_of_the_file_is_the_models_painting_of_the_oracles_maps(tmp_path, kind, mode, caplog):
    from ysmr_amd.track_eval import threshold_video_path
    frames = C.clip(kind)
    plain, _, plain_out, _ = run(tmp_path, "off", frames)
    assert sorted(os.listdir(plain_out)) == ["clip_list.csv"]                          # with the key off, no file is written
    value = {"mask": True, "markers": "Markers", "classes": "CLASSES"}[mode]
    with caplog.at_level(logging.INFO, logger="ysmr"):
        got, path, out, settings = run(tmp_path, "on", frames, **{"hip save threshold video": value})
    written = threshold_video_path(path, out, settings)
    assert written == os.path.join(out, NAME) and written in caplog.text
    assert sorted(os.listdir(out)) == ["clip_list.csv", NAME]
    assert csv_of(out) == csv_of(plain_out) and same_table(got[0], plain[0]) and got[1:4] == plain[1:4]
    count, stored = read_video(written)
    assert count == C.FRAMES
    want = C.expected(kind, mode)
    assert_frames(stored, want)
    if mode == "classes":      # (not an empty overlay: all three colours in one frame, from the oracle's maps)
        assert (C.classes_per_frame(kind) > 0).all(axis=1).any()
        assert all((want == colour).all(axis=3).any(axis=(1, 2)).any() for colour in (T.KEPT_MARKER, T.KEPT, T.DROPPED))


def test_the_mean_gray_branch_shows_its_mask_and_has_no_markers(tmp_path, caplog):
    frames = C.clip("gray")
    keys = {"adaptive double threshold": -1}
    plain, _, plain_out, _ = run(tmp_path, "off", frames, **keys)
    got, _, out, _ = run(tmp_path, "mask", frames, **{"hip save threshold video": "mask"}, **keys)
    count, stored = read_video(os.path.join(out, NAME))
    assert count == C.FRAMES
    assert_frames(stored, C.expected("gray", "mask", -1))
    assert (C.expected("gray", "mask", -1) != C.expected("gray", "mask")).any()       # (another mask than the double threshold's)
    assert same_table(got[0], plain[0]) and csv_of(out) == csv_of(plain_out)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="ysmr"):
        got, _, out, _ = run(tmp_path, "markers", frames, **{"hip save threshold video": "markers"}, **keys)
    warnings = [r for r in caplog.records if "hip save threshold video" in r.getMessage()]
    assert len(warnings) == 1 and warnings[0].levelno == logging.WARNING
    assert sorted(os.listdir(out)) == ["clip_list.csv"]
    assert same_table(got[0], plain[0]) and csv_of(out) == csv_of(plain_out)


def test_both_views_at_once_write_the_files_each_writes_alone(tmp_path):
    frames = C.clip("gray")
    plain, _, plain_out, _ = run(tmp_path, "off", frames)
    thr, _, thr_out, _ = run(tmp_path, "threshold", frames, **{"hip save threshold video": "classes"})
    det, _, det_out, _ = run(tmp_path, "detection", frames, **{"hip save detection video": True})
    both, _, both_out, _ = run(tmp_path, "both", frames, **{"hip save threshold video": "classes", "hip save detection video": True})
    assert sorted(os.listdir(both_out)) == ["clip_detections_output.avi", "clip_list.csv", NAME]
    for got, out in ((thr, thr_out), (det, det_out), (both, both_out)):
        assert csv_of(out) == csv_of(plain_out) and same_table(got[0], plain[0]) and got[1:4] == plain[1:4]
    assert open(os.path.join(both_out, NAME), "rb").read() == open(os.path.join(thr_out, NAME), "rb").read()
    assert open(os.path.join(both_out, "clip_detections_output.avi"), "rb").read() == \
        open(os.path.join(det_out, "clip_detections_output.avi"), "rb").read()


def test_motion_jpeg_chunks_are_the_encoding_of_the_expected_frames(tmp_path):
    import jpeg_model as jm
    frames = C.clip("bgr")
    plain, _, plain_out, _ = run(tmp_path, "off", frames)
    got, _, out, _ = run(tmp_path, "mjpg", frames, **{"hip save threshold video": "classes", "save video fourcc codec": "MJPG",
                                                      "hip video jpeg quality": 85})
    payloads = _payloads(os.path.join(out, NAME))
    want = C.expected("bgr", "classes")
    assert len(payloads) == C.FRAMES
    for i in range(C.FRAMES):
        assert payloads[i] == jm.encode(want[i], 85), "frame {}".format(i)
    assert same_table(got[0], plain[0]) and csv_of(out) == csv_of(plain_out)


def test_an_overflow_rerun_leaves_one_complete_file(tmp_path, caplog):
    frames = C.clip("gray")
    plain, _, _, _ = run(tmp_path, "roomy", frames)
    # eight detections per frame are too few (the oracle counts up to ten): the pass is repeated with doubled buffers
    got, _, out, _ = run(tmp_path, "tight", frames, max_det=8, capacity=8, **{"hip save threshold video": "mask"})
    assert "running it again" in caplog.text
    count, stored = read_video(os.path.join(out, NAME))
    assert count == C.FRAMES and same_table(got[0], plain[0])
    assert_frames(stored, C.expected("gray", "mask"))
    assert sorted(os.listdir(out)) == ["clip_list.csv", NAME]


def test_a_failed_pass_leaves_no_file(tmp_path, caplog, monkeypatch):
    from ysmr_amd import _lib, track_eval
    frames = C.clip("gray")
    target = os.path.join(str(tmp_path / "fails" / "out"), NAME)
    seen = []

    def check(self, res):      # the pipeline's look at its error flags, behind the first linked batch
        seen.append(os.path.isfile(target))
        raise _lib.YsmrLibraryError("made to fail")

    monkeypatch.setattr(track_eval.TrackingPipeline, "check", check)
    run(tmp_path, "fails", frames, expect=False, **{"hip save threshold video": "classes"})
    assert seen == [True] and "made to fail" in caplog.text
    assert not os.path.exists(target)


def test_a_bad_value_or_bad_video_settings_return_none_and_write_nothing(tmp_path, caplog):
    frames = C.clip("gray")
    with caplog.at_level(logging.CRITICAL, logger="ysmr"):
        _, _, out, _ = run(tmp_path, "word", frames, expect=False, **{"hip save threshold video": "thresh"})
    critical = [r for r in caplog.records if r.levelno == logging.CRITICAL]
    assert len(critical) == 1 and "hip save threshold video" in critical[0].getMessage() and "'thresh'" in critical[0].getMessage()
    assert os.listdir(out) == []
    caplog.clear()
    _, _, out, _ = run(tmp_path, "quality", frames, expect=False, **{"hip save threshold video": "mask", "save video fourcc codec": "MJPG",
                                                                     "hip video jpeg quality": 0})
    assert "hip video jpeg quality" in caplog.text and os.listdir(out) == []


def test_a_file_that_cannot_be_opened_ends_the_view_and_tracking_goes_on(tmp_path, caplog):
    from ysmr_amd.track_eval import track_bacteria
    frames = C.clip("gray")
    plain, _, _, _ = run(tmp_path, "plain", frames)
    folder = tmp_path / "blocked"
    (folder / "out" / NAME).mkdir(parents=True)          # a directory where the file is to go
    np.save(folder / "clip.npy", frames)
    for codec in ("DIB ", "MJPG"):
        s = _settings(**{"hip save threshold video": "mask", "save video fourcc codec": codec})
        got = track_bacteria(str(folder / "clip.npy"), settings=s, result_folder=str(folder / "out"), batch=C.BATCH, max_det=256, capacity=256)
        assert got is not None and same_table(got[0], plain[0])
    assert caplog.text.count("is not written") == 2
    assert os.path.isdir(str(folder / "out" / NAME))
