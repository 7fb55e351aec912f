"""``ysmr_view_boxes_batch`` and ``ysmr_view_tracks_batch`` on the device against the sequential painter of
tests/view_model.py, on the cases of tests/test_view_cpu.py: every output byte must be equal."""
import functools

import numpy as np
import pytest

import annotate_model as A
import view_model as V

pytestmark = pytest.mark.gpu

FIRST = 1000          # the batch begins at this frame of its video
FILL, GAP = 0xA5, 12


@functools.lru_cache(maxsize=None)
def case(channels):
    """Frames, detections, the rows as the device gets them (a slice of a longer array, in no frame order) and the model's
    painted frames: computed once, never modified."""
    frames = V.frames_of(channels)
    det, det_count, rows = V.cases(FIRST)
    rows = rows[np.random.default_rng(3).permutation(len(rows))]
    longer = np.concatenate([np.array([V.row(FIRST + 1, 77, 40.0, 30.0)] * 3, V.ROW_DTYPE), rows,
                             np.array([V.row(FIRST + 2, 78, 20.0, 20.0)] * 2, V.ROW_DTYPE)])
    painted = V.paint(frames, det, det_count, rows, FIRST)
    boxes_only = V.paint(frames, det, det_count, rows[:0], FIRST)
    for a in (frames, det, det_count, longer, painted, boxes_only):
        a.setflags(write=False)
    return frames, det, det_count, longer, (3, 3 + len(rows)), painted, boxes_only


def launch(frames, det, det_count, rows, span, bottom_up, tracks=True, stride=None):
    import torch
    from ysmr_amd import _lib
    n, h, w = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    stride = (3 * w + 3) & ~3 if stride is None else stride
    frame_bytes = stride * h + GAP
    dev = torch.device("cuda:0")
    L = _lib.lib()
    frames_dev = torch.from_numpy(np.array(frames)).to(dev)
    det_dev = torch.from_numpy(np.array(det)).to(dev)
    count_dev = torch.from_numpy(np.array(det_count)).to(dev)
    rows_dev = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).to(dev)
    span_dev = torch.tensor(span, dtype=torch.int64, device=dev)
    out = torch.full((n, frame_bytes), FILL, dtype=torch.uint8, device=dev)
    _lib.check(L.ysmr_view_boxes_batch(_lib.stream_ptr(dev), frames_dev.data_ptr(), n, h, w, ch, det_dev.data_ptr(), count_dev.data_ptr(),
                                       det.shape[1], out.data_ptr(), stride, frame_bytes, int(bottom_up)), "ysmr_view_boxes_batch")
    if tracks:
        _lib.check(L.ysmr_view_tracks_batch(_lib.stream_ptr(dev), rows_dev.data_ptr(), len(rows), span_dev.data_ptr(), span_dev.data_ptr() + 8,
                                            FIRST, n, h, w, out.data_ptr(), stride, frame_bytes, int(bottom_up)), "ysmr_view_tracks_batch")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


@pytest.mark.parametrize("bottom_up", [1, 0])
@pytest.mark.parametrize("channels", [1, 3])
def test_both_layers_equal_the_sequential_painter(channels, bottom_up):
    frames, det, det_count, rows, span, painted, boxes_only = case(channels)
    stride = (3 * V.W + 3) & ~3
    got = launch(frames, det, det_count, rows, span, bottom_up)
    want = A.pack_dib(painted, bottom_up, frame_bytes=stride * V.H + GAP, fill=FILL)
    for i in range(V.N):
        assert np.array_equal(got[i], want[i]), "frame {}: {} bytes differ".format(i, int((got[i] != want[i]).sum()))
    half = launch(frames, det, det_count, rows, span, bottom_up, tracks=False)
    assert np.array_equal(half, A.pack_dib(boxes_only, bottom_up, frame_bytes=stride * V.H + GAP, fill=FILL))
    assert (painted != boxes_only).any() and (boxes_only != A.to_bgr(frames)).any()
    assert np.array_equal(painted[2], A.to_bgr(frames)[2])


def test_padding_is_zeroed_and_nothing_else_is_touched():
    frames, det, det_count, rows, span, painted, _ = case(1)
    stride = (3 * V.W + 3) & ~3
    assert stride > 3 * V.W
    got = launch(frames, det, det_count, rows, span, 1)
    stored = got[:, :stride * V.H].reshape(V.N, V.H, stride)
    assert (stored[:, :, 3 * V.W:] == 0).all()
    assert (got[:, stride * V.H:] == FILL).all()                    # the bytes between two frames are the caller's
    wide = launch(frames, det, det_count, rows, span, 0, stride=stride + 8).reshape(V.N, -1)[:, :(stride + 8) * V.H]
    wide = wide.reshape(V.N, V.H, stride + 8)
    assert (wide[:, :, 3 * V.W:] == 0).all()
    assert np.array_equal(wide[:, :, :3 * V.W].reshape(V.N, V.H, V.W, 3), painted)


def test_an_empty_and_a_cut_row_range_paint_what_they_name():
    frames, det, det_count, rows, span, painted, boxes_only = case(1)
    assert np.array_equal(launch(frames, det, det_count, rows, (5, 5), 0)[:, :-GAP], A.pack_dib(boxes_only, 0))
    # a counter beyond the array (a row buffer that overflowed) is cut to it: the rows in front are painted, nothing is read behind
    cut = launch(frames, det, det_count, rows[:span[1]], (span[0], span[1] + 1000), 0)
    assert np.array_equal(cut[:, :-GAP], A.pack_dib(painted, 0))


def test_two_runs_give_the_same_bytes():
    frames, det, det_count, rows, span, _, _ = case(3)
    a = launch(frames, det, det_count, rows, span, 1)
    b = launch(frames, det, det_count, rows, span, 1)
    assert np.array_equal(a, b)


def test_the_host_twin_and_the_device_agree_on_random_boxes():
    """Many boxes per frame (more than one slice of a frame's detections, more than one workgroup), against the host twin,
    which tests/test_view_cpu.py holds to the model."""
    from test_view_cpu import host_view
    rng = np.random.default_rng(8)
    n, h, w, m = 5, 61, 83, 300
    frames = rng.integers(0, 200, (n, h, w), dtype=np.uint8)
    det = np.zeros((n, m, 5), np.float32)
    det[..., 0] = rng.uniform(-8, w + 8, (n, m))
    det[..., 1] = rng.uniform(-8, h + 8, (n, m))
    det[..., 2] = rng.choice([0, 1, 2, 3.5, 7, 12.3, 30], (n, m))
    det[..., 3] = rng.choice([0, 1, 2.2, 4, 9, 21], (n, m))
    det[..., 4] = np.where(rng.integers(0, 3, (n, m)) == 0, rng.choice([0, 90, -90], (n, m)), rng.uniform(-90, 90, (n, m)))
    det_count = np.array([m, 0, 17, 250, 1], np.int32)
    rows = np.zeros(600, V.ROW_DTYPE)
    rows["frame"] = FIRST + rng.integers(-1, n + 1, 600)
    rows["track_id"] = rng.integers(0, 100000, 600)
    rows["x"], rows["y"] = rng.uniform(-15, w + 15, 600), rng.uniform(-15, h + 25, 600)
    got = launch(frames, det, det_count, rows, (0, 600), 1)
    want = host_view(frames, det, det_count, rows, FIRST, 1, frame_bytes=((3 * w + 3) & ~3) * h + GAP, fill=FILL)
    assert np.array_equal(got, want)
