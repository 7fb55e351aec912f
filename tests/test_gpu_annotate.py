"""``ysmr_annotate_batch`` and ``annotate_video`` on the device against the sequential painter of tests/annotate_model.py:
every output byte must be equal."""
import functools
import os

import numpy as np
import pytest

import annotate_model as am

pytestmark = pytest.mark.gpu

SHAPES = {"gray37x50": (37, 50, 1), "gray16x40": (16, 40, 1), "bgr23x41": (23, 41, 3)}      # H, W, channels
COUNTS = (0, 1, 65, 200, 3)                                                                  # marks per frame
BIG_ID = 4294967295


def _mark(x, y, track_id, style):
    return (int(x), int(y), int(track_id), int(style))


def _random_marks(rng, n, h, w):
    ids = np.where(rng.random(n) < 0.2, rng.integers(0, 10, n),
                   np.where(rng.random(n) < 0.5, rng.integers(10, 1000, n), rng.integers(1000, BIG_ID + 1, n)))
    return [_mark(rng.integers(-20, w + 20), rng.integers(-20, h + 25), ids[k], rng.integers(0, 3)) for k in range(n)]


def _busy_frame(rng, h, w):
    """The 200 marks: ids of 1, 2 and 10 digits, the three styles, text and dots cut by each edge and outside on each
    side, 70 marks within 3 px of each other (a later-mark scan of more than 64), two identical marks."""
    marks = [
        _mark(w // 2, h // 2, 5, 0), _mark(w // 3, h // 2 + 4, 42, 1), _mark(12, h - 2, BIG_ID, 2),
        # cut by the left, right, top and bottom edge: the text, then a large dot
        _mark(3, h // 2, 123, 0), _mark(0, h // 2 + 3, 8, 2),
        _mark(w - 4, h // 2, BIG_ID, 1), _mark(w - 1, h // 2 - 3, 9, 2),
        _mark(w // 2, 10, 77, 0), _mark(w // 2 + 9, 0, 6, 2),
        _mark(w // 2, h + 12, 31, 1), _mark(w // 2 - 9, h - 1, 4, 2),
        # entirely outside on each side, negative coordinates and the ends of int32 among them
        _mark(-100, 5, 11, 0), _mark(w + 100, 5, 12, 1), _mark(5, -100, 13, 2), _mark(5, h + 100, 14, 0),
        _mark(-2, h // 2, 15, 2), _mark(w // 2, -2, 16, 2), _mark(w + 1, 3, 17, 2), _mark(4, h + 1, 18, 2),
        _mark(-2147483648, 2147483647, BIG_ID, 2), _mark(2147483647, -2147483648, BIG_ID, 2),
    ]
    cx, cy = w // 2 + 2, h // 2 + 9
    marks += [_mark(cx + rng.integers(0, 3), cy + rng.integers(0, 3), rng.integers(0, 1000), k % 3) for k in range(70)]
    marks += [_mark(w // 4, h // 2 + 6, 808, 2)] * 2
    marks += _random_marks(rng, 200 - len(marks), h, w)
    order = rng.permutation(len(marks))                      # (the stack and the edge cases mixed through the table)
    return [marks[k] for k in order]


@functools.lru_cache(maxsize=None)
def case(name):
    """Frames, marks, first and the model's painted frames of one shape: computed once, never modified."""
    h, w, ch = SHAPES[name]
    rng = np.random.default_rng(sorted(SHAPES).index(name))
    frames = rng.integers(0, 256, (len(COUNTS), h, w) + ((3,) if ch == 3 else ()), dtype=np.uint8)
    per_frame = [[], [_mark(w // 2, h // 2, 7, 2)], _random_marks(rng, 65, h, w), _busy_frame(rng, h, w),
                 [_mark(11, 17, 0, 0), _mark(13, 18, 10, 1), _mark(w - 2, h - 2, 99, 2)]]
    assert tuple(len(m) for m in per_frame) == COUNTS
    marks = np.array([m for frame in per_frame for m in frame], dtype=am.MARK_DTYPE)
    first = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    painted = am.paint(frames, marks, first)
    for a in (frames, marks, first, painted):
        a.setflags(write=False)
    return frames, marks, first, painted


def launch(frames, marks, first, bottom_up, gap=12, fill=0xAA, stride=None):
    """One ``ysmr_annotate_batch`` into a buffer pre-filled with ``fill``, frames ``stride * H + gap`` bytes apart."""
    import torch
    from ysmr_amd import _lib
    n, h, w = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    stride = (3 * w + 3) & ~3 if stride is None else stride
    frame_bytes = stride * h + gap
    dev = torch.device("cuda:0")
    frames_dev = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    out = torch.full((n, frame_bytes), fill, dtype=torch.uint8, device=dev)
    marks_dev = first_dev = None
    if first is not None:
        padded = np.zeros(max(1, len(marks)), am.MARK_DTYPE)
        padded[:len(marks)] = marks
        marks_dev = torch.from_numpy(padded.view(np.uint8).reshape(-1)).to(dev)
        first_dev = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int64)).to(dev)
    rc = _lib.lib().ysmr_annotate_batch(_lib.stream_ptr(dev), frames_dev.data_ptr(), n, h, w, ch,
                                        None if marks_dev is None else marks_dev.data_ptr(),
                                        None if first_dev is None else first_dev.data_ptr(), out.data_ptr(), stride,
                                        frame_bytes, int(bottom_up))
    _lib.check(rc, "ysmr_annotate_batch")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


@pytest.mark.parametrize("bottom_up", [1, 0])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_painted_frames_equal_the_sequential_painter(name, bottom_up):
    frames, marks, first, painted = case(name)
    h, w = frames.shape[1:3]
    got = launch(frames, marks, first, bottom_up)
    want = am.pack_dib(painted, bottom_up, frame_bytes=((3 * w + 3) & ~3) * h + 12, fill=0xAA)
    for i in range(len(COUNTS)):
        assert np.array_equal(got[i], want[i]), "frame {} ({} marks): {} bytes differ".format(
            i, COUNTS[i], int((got[i] != want[i]).sum()))
    # the marks did something, and in every style's colour
    assert (painted != am.to_bgr(frames)).any(axis=(1, 2, 3)).tolist() == [False, True, True, True, True]
    for colour in am.COLOURS.values():
        assert (painted[3] == np.array(colour, np.uint8)).all(axis=2).any()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_padding_is_zeroed_and_nothing_else_is_touched(name):
    frames, marks, first, _ = case(name)
    h, w = frames.shape[1:3]
    stride = (3 * w + 3) & ~3
    got = launch(frames, marks, first, 1, gap=12, fill=0xAA)
    rows = got[:, :stride * h].reshape(len(frames), h, stride)
    assert (rows[:, :, 3 * w:] == 0).all()                   # (no padding at W = 40: an empty slice)
    assert (got[:, stride * h:] == 0xAA).all()               # the bytes between two frames are the caller's
    wide = launch(frames, marks, first, 0, gap=0, fill=0xAA, stride=stride + 8)     # a stride of the caller's choosing
    rows = wide.reshape(len(frames), h, stride + 8)
    assert (rows[:, :, 3 * w:] == 0).all()
    assert np.array_equal(rows[:, :, :3 * w], got[:, :stride * h].reshape(len(frames), h, stride)[:, ::-1, :3 * w])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_without_marks_the_frames_are_only_packed(name):
    frames, _, _, _ = case(name)
    for bottom_up in (1, 0):
        got = launch(frames, None, None, bottom_up, gap=0)
        assert np.array_equal(got, am.pack_dib(am.to_bgr(frames), bottom_up))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_busy_frame_eight_times_in_one_launch_gives_eight_identical_images(name):
    frames, marks, first, painted = case(name)
    busy = marks[first[3]:first[4]]
    eight = np.repeat(frames[3:4], 8, axis=0)
    got = launch(eight, np.tile(busy, 8), np.arange(9, dtype=np.int64) * len(busy), 1, gap=0)
    for i in range(1, 8):
        assert np.array_equal(got[i], got[0]), "frame {} differs from frame 0".format(i)
    assert np.array_equal(got[0], am.pack_dib(painted[3:4], 1)[0])


def test_first_may_point_into_a_longer_array():
    """A batch in the middle of a video: first[0] is not 0, the marks before it belong to earlier frames."""
    import torch
    from ysmr_amd import _lib
    frames, marks, first, painted = case("gray37x50")
    h, w = frames.shape[1:3]
    dev = torch.device("cuda:0")
    frames_dev = torch.from_numpy(np.ascontiguousarray(frames[2:4])).to(dev)
    marks_dev = torch.from_numpy(marks.view(np.uint8).reshape(-1).copy()).to(dev)
    first_dev = torch.from_numpy(first.copy()).to(dev)
    stride = (3 * w + 3) & ~3
    out = torch.zeros((2, stride * h), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().ysmr_annotate_batch(_lib.stream_ptr(dev), frames_dev.data_ptr(), 2, h, w, 1, marks_dev.data_ptr(),
                                              first_dev.data_ptr() + 8 * 2, out.data_ptr(), stride, stride * h, 1),
               "ysmr_annotate_batch")
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy(), am.pack_dib(painted[2:4], 1))


# ---- end to end ------------------------------------------------------------------------------------------------------

def _clip_and_table():
    """A 12-frame 48 x 64 gray clip, and an evaluated table of seven tracks in the order evaluate_tracks leaves it
    (by TRACK_ID, then POSITION_T), with the marks it must give, frame by frame, written down beside it."""
    import pandas as pd
    rng = np.random.default_rng(12)
    clip = rng.integers(0, 200, (12, 48, 64), dtype=np.uint8)
    rows, per_frame = [], [[] for _ in range(12)]
    for track, phenotype in ((3, 2), (12, 0), (345, 2), (6789, 1), (70000, 2), (4000000000, 2), (5, 0)):
        x, y = float(rng.integers(5, 60)), float(rng.integers(10, 45))
        for t in range(int(rng.integers(0, 3)), 12 - int(rng.integers(0, 3))):
            x, y = x + rng.uniform(-2.5, 2.5), y + rng.uniform(-2.5, 2.5)
            moving = 0 if phenotype == 0 else int(rng.random() < 0.8)
            turn = int(rng.random() < 0.3)
            rows.append((track, t, x, y, moving, turn, phenotype))
            per_frame[t].append((int(x), int(y), track, 1 if moving == 0 else 2 if turn == 1 else 0, phenotype))
    rows.sort(key=lambda r: (r[0], r[1]))
    for marks in per_frame:
        marks.sort(key=lambda m: m[2])
    df = pd.DataFrame(rows, columns=["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "moving", "turn_points",
                                     "motility_phenotype"])
    df = df.astype({"TRACK_ID": np.int64, "POSITION_T": np.int64, "moving": np.int8, "turn_points": np.int8,
                    "motility_phenotype": np.int8})
    return clip, df, per_frame


def _expected(clip, per_frame, subtype=None):
    kept = [[m[:4] for m in marks if subtype is None or m[4] == subtype] for marks in per_frame]
    marks = np.array([m for frame in kept for m in frame], dtype=am.MARK_DTYPE)
    first = np.concatenate([[0], np.cumsum([len(f) for f in kept])]).astype(np.int64)
    return am.paint(clip, marks, first)


@pytest.mark.parametrize("container", ["npy", "avi"])
def test_annotate_video_end_to_end(tmp_path, container, caplog):
    from avi_tools import write_avi
    from ysmr_amd import annotate_video
    from ysmr_amd.frames import AviVideo
    from ysmr_amd.helper_file import default_settings
    clip, df, per_frame = _clip_and_table()
    if container == "npy":
        path = str(tmp_path / "clip.npy")
        np.save(path, clip)
    else:
        path = str(tmp_path / "clip.avi")
        write_avi(path, am.to_bgr(clip), bits=24, fps=(25, 1))
    out = str(tmp_path / "results")
    s = default_settings(**{"log to file": False, "hip frames per batch": 5, "frames per second": 25.0})
    written = annotate_video(path, df, settings=s, result_folder=out)          # three batches: 5, 5 and 2 frames
    assert written == os.path.join(out, "clip_annotated_output.avi") and os.path.isfile(written)
    assert "uncompressed 24-bit AVI" in caplog.text                            # (the settings ask for .mp4 / mp4v)
    video = AviVideo(written)
    assert (video.frame_count, video.frames_available, video.height, video.width, video.channels) == (12, 12, 48, 64, 3)
    assert video.fps == 25.0
    got = video.read(0, 12)
    video.close()
    want = _expected(clip, per_frame)
    for i in range(12):
        assert np.array_equal(got[i], want[i]), "frame {}".format(i)
    assert (want != am.to_bgr(clip)).any()

    written = annotate_video(path, df, settings=s, result_folder=out, select_subtype=2)
    assert written == os.path.join(out, "motile_subtype_clip_annotated_output.avi")
    video = AviVideo(written)
    got = video.read(0, 12)
    video.close()
    want_motile = _expected(clip, per_frame, subtype=2)
    assert np.array_equal(got, want_motile) and (want_motile != want).any()
    assert sorted(os.listdir(out)) == ["clip_annotated_output.avi", "motile_subtype_clip_annotated_output.avi"]
