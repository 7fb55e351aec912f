"""The detection view where there is no GPU: ``ysmr_view_batch_host`` -- the code that decides a pixel in csrc/view.hip's
kernels, run on host arrays -- against the sequential painter of tests/view_model.py, byte for byte; the model's own
short cut for far-away segments against ``line8``; the settings key and the file name."""
import time

import numpy as np
import pytest

import annotate_model as A
import luminosity_model as M
import view_model as V

from ysmr_amd import _lib


def host_view(frames, det, det_count, rows, first, bottom_up, stride=None, frame_bytes=None, fill=0xA5, begin=0, end=None):
    n, H, W = frames.shape[:3]
    channels = 1 if frames.ndim == 3 else 3
    stride = (3 * W + 3) & ~3 if stride is None else stride
    frame_bytes = stride * H if frame_bytes is None else frame_bytes
    out = np.full((n, frame_bytes), fill, np.uint8)
    frames, det, det_count, rows = (np.ascontiguousarray(a) for a in (frames, det, det_count, rows))
    end = len(rows) if end is None else end
    rc = _lib.lib().ysmr_view_batch_host(frames.ctypes.data, n, H, W, channels, det.ctypes.data, det_count.ctypes.data, det.shape[1],
                                         rows.ctypes.data if len(rows) else None, begin, end, first, out.ctypes.data, stride,
                                         frame_bytes, bottom_up)
    _lib.check(rc, "ysmr_view_batch_host")
    return out


def test_the_short_cut_for_far_segments_is_line8():
    """view_model.line8_window (used only where walking is out of the question) gives exactly line8's pixels in the frame."""
    rng = np.random.default_rng(11)
    H, W = 23, 31
    for _ in range(3000):
        span = int(rng.choice([3, 40, 400]))
        p = (int(rng.integers(-span, W + span)), int(rng.integers(-span, H + span)))
        q = (int(rng.integers(-span, W + span)), int(rng.integers(-span, H + span)))
        if rng.integers(0, 6) == 0:
            q = (q[0], p[1]) if rng.integers(0, 2) else (p[0], q[1])
        walked = {(x, y) for (x, y) in M.line8(p, q) if 0 <= x < W and 0 <= y < H}
        assert V.line8_window(p, q, H, W) == walked, (p, q)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("bottom_up", [0, 1])
def test_host_twin_paints_what_the_model_paints(channels, bottom_up):
    first = 0
    frames = V.frames_of(channels)
    det, det_count, rows = V.cases(first)
    stride = (3 * V.W + 3) & ~3
    assert stride != 3 * V.W
    want = A.pack_dib(V.paint(frames, det, det_count, rows, first), bottom_up, stride, stride * V.H + 12, fill=0xA5)
    got = host_view(frames, det, det_count, rows, first, bottom_up, stride, stride * V.H + 12)
    assert np.array_equal(got, want)
    painted = want[:, :stride * V.H].reshape(V.N, V.H, stride)[:, :, :3 * V.W].reshape(V.N, V.H, V.W, 3)
    if bottom_up:
        painted = painted[:, ::-1]
    base = A.to_bgr(frames)
    assert np.array_equal(painted[2], base[2])                        # the frame with no detection and no row
    blue = (painted == (255, 0, 0)).all(axis=3)
    green = (painted == (0, 255, 0)).all(axis=3)
    assert blue[0].sum() > 200 and green[1].sum() > 200 and blue[1].sum() > 20 and green[0].sum() > 10
    # the digits of id 7 at (30, 24) start at (20, 8), seven rows: they cross the lower edge (y = 16 / 15) of the box under them
    assert green[1, 8:15, 20:25].sum() > 5


def test_boxes_with_corners_a_million_pixels_away_cost_what_near_boxes_cost():
    """The work of a segment is bounded by the frame, not by its corners.  The same call with the five far boxes of the table
    and with five boxes inside the frame, the packing being the same in both; of five runs each the fastest counts, so that
    a busy machine cannot fail it.  Walking the far boxes' edges would be some 10^7 steps, a thousand times the near ones';
    the bound leaves a factor of 20 and two milliseconds."""
    frames = V.frames_of(1)
    det, det_count, _ = V.cases(0)
    far = det[0, 17:22]
    assert all(max(abs(v) for p in M.int_corners(d) for v in p) >= 300000 for d in far)
    near = det[0, 0:5]
    none = np.zeros(0, V.ROW_DTYPE)

    def fastest(boxes):
        d = np.zeros((V.N, 5, 5), np.float32)
        d[:] = boxes
        best = float("inf")
        for _ in range(5):
            t0 = time.perf_counter()
            host_view(frames, d, np.full(V.N, 5, np.int32), none, 0, 0)
            best = min(best, time.perf_counter() - t0)
        return best

    t_near, t_far = fastest(near), fastest(far)
    assert t_far < 20 * t_near + 0.002, (t_near, t_far)


def test_green_wins_over_blue_where_they_meet():
    frames = np.zeros((1, V.H, V.W), np.uint8)
    det = np.array([[(24.0, 12.0, 30.0, 8.0, 0.0)]], np.float32)
    rows = np.array([V.row(0, 8, 30.0, 24.0)], V.ROW_DTYPE)
    only_box = V.paint(frames, det, np.array([1], np.int32), rows[:0], 0)
    both = V.paint(frames, det, np.array([1], np.int32), rows, 0)
    meet = (only_box[0] == (255, 0, 0)).all(axis=2) & (both[0] == (0, 255, 0)).all(axis=2)
    assert meet.sum() >= 2                                            # (the case is what it claims to be)
    got = host_view(frames, det, np.array([1], np.int32), rows, 0, 0)
    assert np.array_equal(got, A.pack_dib(both, 0))


def test_rows_are_a_slice_and_their_frames_are_relative_to_the_batch():
    first = 1000
    frames = V.frames_of(1, seed=6)
    det, det_count, rows = V.cases(first)
    rng = np.random.default_rng(2)
    rows = rows[rng.permutation(len(rows))]                           # no frame order
    longer = np.concatenate([np.array([V.row(first + 1, 77, 40.0, 30.0)] * 3, V.ROW_DTYPE), rows,
                             np.array([V.row(first + 2, 78, 20.0, 20.0)] * 2, V.ROW_DTYPE)])
    got = host_view(frames, det, det_count, longer, first, 1, begin=3, end=3 + len(rows))
    assert np.array_equal(got, A.pack_dib(V.paint(frames, det, det_count, rows, first), 1))
    none = host_view(frames, det, det_count, longer, first, 1, begin=5, end=5)
    assert np.array_equal(none, A.pack_dib(V.paint(frames, det, det_count, rows[:0], first), 1))


def test_every_outline_pixel_lies_in_the_fill_of_the_same_corners():
    """The outline is the fill's own edge set: luminosity_model.fill begins with these lines."""
    rng = np.random.default_rng(4)
    H, W = 40, 56
    n = 400
    det = np.zeros((1, n, 5), np.float32)
    det[0, :, 0] = rng.uniform(-6, W + 6, n)
    det[0, :, 1] = rng.uniform(-6, H + 6, n)
    det[0, :, 2] = rng.choice([0, 1, 2, 3.5, 7, 12.3, 20], n)
    det[0, :, 3] = rng.choice([0, 1, 2.2, 4, 9, 17], n)
    det[0, :, 4] = np.where(rng.integers(0, 3, n) == 0, rng.choice([0, 90, -90], n), rng.uniform(-90, 90, n))
    zero = np.zeros((1, H, W), np.uint8)
    for d in range(n):
        got = host_view(zero, det[:, d:d + 1], np.array([1], np.int32), np.zeros(0, V.ROW_DTYPE), 0, 0)
        img = got.reshape(H, -1)[:, :3 * W].reshape(H, W, 3)
        ys, xs = np.nonzero((img == (255, 0, 0)).all(axis=2))
        pts = M.int_corners(det[0, d])
        assert set(zip(xs.tolist(), ys.tolist())) == V.outline(pts, H, W), det[0, d]
        assert set(zip(xs.tolist(), ys.tolist())) <= M.fill(pts, H, W), det[0, d]
        assert img[~(img == (255, 0, 0)).all(axis=2)].sum() == 0


def test_bad_arguments_are_refused():
    frames = V.frames_of(1)
    det, det_count, rows = V.cases(0)
    L = _lib.lib()
    out = np.zeros((V.N, 152 * V.H), np.uint8)
    args = lambda **kw: [kw.get("frames", frames.ctypes.data), V.N, V.H, V.W, kw.get("channels", 1), det.ctypes.data, det_count.ctypes.data,
                         det.shape[1], rows.ctypes.data, 0, len(rows), 0, out.ctypes.data, kw.get("stride", 152), kw.get("fb", 152 * V.H), 0]
    assert L.ysmr_view_batch_host(*args()) == _lib.YSMR_OK
    assert L.ysmr_view_batch_host(*args(channels=2)) == _lib.YSMR_ERR_ARG
    assert L.ysmr_view_batch_host(*args(stride=150)) == _lib.YSMR_ERR_ARG          # 3 * 50, not a multiple of 4
    assert L.ysmr_view_batch_host(*args(fb=152 * V.H - 4)) == _lib.YSMR_ERR_ARG
    assert L.ysmr_view_batch_host(*args(frames=None)) == _lib.YSMR_ERR_ARG


def test_the_settings_key_and_the_file_name(tmp_path):
    from ysmr_amd.helper_file import create_configs, default_settings, get_configs
    from ysmr_amd.track_eval import detection_video_path
    assert "hip save detection video" not in default_settings()
    ini = tmp_path / "tracking.ini"
    create_configs(str(ini))
    assert "hip save detection video" not in get_configs(str(ini))     # a tracking.ini without the key reads as before
    text = ini.read_text().replace("[ADVANCED VIDEO SETTINGS]", "[ADVANCED VIDEO SETTINGS]\nhip save detection video = True")
    ini.write_text(text)
    assert get_configs(str(ini))["hip save detection video"] is True
    s = default_settings()
    assert detection_video_path("/data/run 3/clip.01.avi", str(tmp_path), s) == str(tmp_path / "clip.01_detections_output.avi")
