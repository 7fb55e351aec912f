"""``ysmr_mjpeg_batch`` and ``annotate_video`` in Motion-JPEG mode on the device against the model of tests/jpeg_model.py:
every byte of every chunk must be equal."""
import functools
import io
import logging
import os
import struct

import numpy as np
import pytest

import annotate_model as am
import jpeg_model as jm
from test_mjpeg_cpu import checkerboard, saturated

pytestmark = pytest.mark.gpu

SHAPES = ((8, 8), (9, 17), (37, 50), (16, 40), (23, 41), (24, 539))
QUALITIES = (1, 50, 90, 100)
_PAINTED = {(37, 50): "gray37x50", (16, 40): "gray16x40", (23, 41): "bgr23x41"}


@functools.lru_cache(maxsize=None)
def frames_of(shape):
    """The frames of one shape, uint8 [n, H, W, 3] (B, G, R): flat, noise, saturated, checkerboard, and, for the shapes of
    the annotate tests, the busy frame as their model painted it.  Computed once, never modified."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    frames = [np.full((h, w, 3), 77, np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), saturated(h, w), checkerboard(h, w)]
    if shape in _PAINTED:
        from test_gpu_annotate import case
        frames.append(np.array(case(_PAINTED[shape])[3][3]))
    out = np.stack(frames)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def chunks_of(shape, quality):
    """The model's chunks of frames_of(shape)."""
    return tuple(jm.chunk(jm.encode(f, quality)) for f in frames_of(shape))


def launch(frames, quality, bottom_up, stride=None, gap=0, capacity=None, guard=64):
    """One ``ysmr_mjpeg_batch``: (out bytes with the guard, offsets [n + 1], status)."""
    import torch
    from ysmr_amd import _lib
    n, h, w = frames.shape[:3]
    stride = (3 * w + 3) & ~3 if stride is None else stride
    frame_bytes = stride * h + gap
    dib = am.pack_dib(frames, bottom_up, stride=stride, frame_bytes=frame_bytes, fill=0x5C)
    dev = torch.device("cuda:0")
    L = _lib.lib()
    ws_bytes = L.ysmr_mjpeg_workspace_bytes(n, h, w)
    dib_dev = torch.from_numpy(np.ascontiguousarray(dib)).to(dev)
    ws = torch.full((ws_bytes,), 0xEE, dtype=torch.uint8, device=dev)          # (the kernels may rely on nothing in it)
    capacity = n * stride * h if capacity is None else capacity
    out = torch.full((capacity + guard,), 0xAA, dtype=torch.uint8, device=dev)
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = L.ysmr_mjpeg_batch(_lib.stream_ptr(dev), dib_dev.data_ptr(), n, h, w, stride, frame_bytes, int(bottom_up), quality,
                            ws.data_ptr(), ws_bytes, out.data_ptr(), capacity, offsets.data_ptr(), status.data_ptr())
    _lib.check(rc, "ysmr_mjpeg_batch")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), offsets.cpu().numpy(), int(status.item())


def _assert_chunks(out, offsets, want, what):
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want])]).tolist(), what
    for i, chunk in enumerate(want):
        got = out[offsets[i]:offsets[i + 1]].tobytes()
        if got != chunk:
            first = next(k for k in range(min(len(got), len(chunk))) if got[k] != chunk[k])
            raise AssertionError("{}: chunk {} differs from byte {} of {} (got {}, want {})".format(
                what, i, first, len(chunk), got[first:first + 8].hex(), chunk[first:first + 8].hex()))


@pytest.mark.parametrize("bottom_up", [1, 0])
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_chunks_equal_the_model_byte_for_byte(shape, quality, bottom_up):
    frames, want = frames_of(shape), chunks_of(shape, quality)
    capacity = max(len(frames) * ((3 * shape[1] + 3) & ~3) * shape[0], sum(len(c) for c in want))
    out, offsets, status = launch(frames, quality, bottom_up, capacity=capacity)
    assert status == 0
    _assert_chunks(out, offsets, want, "{} q{} bottom_up={}".format(shape, quality, bottom_up))
    assert (out[offsets[-1]:] == 0xAA).all()                                   # nothing behind the last chunk


def test_a_stride_and_a_gap_of_the_callers_choosing():
    shape = (23, 41)
    frames, want = frames_of(shape), chunks_of(shape, 90)
    stride = ((3 * 41 + 3) & ~3) + 8
    out, offsets, status = launch(frames, 90, 0, stride=stride, gap=12, capacity=sum(len(c) for c in want))
    assert status == 0
    _assert_chunks(out, offsets, want, "stride + 8, gap 12")


def test_the_noise_frame_eight_times_gives_eight_identical_chunks():
    shape = (37, 50)
    eight = np.repeat(frames_of(shape)[1:2], 8, axis=0)
    want = chunks_of(shape, 90)[1]
    out, offsets, status = launch(eight, 90, 1)
    assert status == 0
    _assert_chunks(out, offsets, (want,) * 8, "eight noise frames")


def test_capacity_contract():
    shape = (23, 41)
    noise = np.stack([np.random.default_rng(k).integers(0, 256, shape + (3,), dtype=np.uint8) for k in range(4)])
    want = tuple(jm.chunk(jm.encode(f, 100)) for f in noise)
    raw = 4 * ((3 * 41 + 3) & ~3) * 23
    total = sum(len(c) for c in want)
    assert total > raw                                                         # (the model says so: noise at quality 100 grows)
    out, offsets, status = launch(noise, 100, 1, capacity=raw)
    assert status & 1
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want])]).tolist()
    assert (out[raw:] == 0xAA).all() and len(out) == raw + 64
    inside = [i for i in range(4) if offsets[i + 1] <= raw]
    assert inside and len(inside) < 4
    for i in inside:
        assert out[offsets[i]:offsets[i + 1]].tobytes() == want[i]
    cut = len(inside)                                                          # the chunk the capacity cuts: right as far as it goes
    assert out[offsets[cut]:raw].tobytes() == want[cut][:raw - offsets[cut]]
    out, offsets, status = launch(noise, 100, 1, capacity=total)
    assert status == 0
    _assert_chunks(out, offsets, want, "exact capacity")
    assert (out[total:] == 0xAA).all()


def test_bad_arguments_are_refused():
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    ws_bytes = L.ysmr_mjpeg_workspace_bytes(1, 16, 24)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    meta = torch.zeros(4, dtype=torch.int64, device=dev)
    good = dict(dib=buf.data_ptr(), n=1, h=16, w=24, stride=72, frame_bytes=72 * 16, quality=90, ws=ws.data_ptr(), ws_bytes=ws_bytes,
                out=buf.data_ptr() + 4096, cap=8192, offsets=meta.data_ptr(), status=meta.data_ptr() + 16)

    def call(**change):
        a = dict(good, **change)
        return L.ysmr_mjpeg_batch(_lib.stream_ptr(dev), a["dib"], a["n"], a["h"], a["w"], a["stride"], a["frame_bytes"], 1, a["quality"],
                                  a["ws"], a["ws_bytes"], a["out"], a["cap"], a["offsets"], a["status"])

    for change in (dict(dib=None), dict(ws=None), dict(out=None), dict(offsets=None), dict(status=None), dict(quality=0),
                   dict(quality=101), dict(stride=70), dict(stride=68), dict(ws_bytes=ws_bytes - 1), dict(n=0)):
        assert call(**change) == _lib.YSMR_ERR_ARG, change
    assert call() == _lib.YSMR_OK
    torch.cuda.synchronize(dev)
    assert int(meta[2].item()) == 0 and int(meta[1].item()) == len(jm.chunk(jm.encode(np.zeros((16, 24, 3), np.uint8), 90)))


# ---- end to end ------------------------------------------------------------------------------------------------------

def _payloads(path):
    """The payloads of the '00dc' chunks of an AVI file, in file order (all RIFF segments)."""
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


def _decode(jpeg):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))[..., ::-1]


def test_annotate_video_writes_motion_jpeg(tmp_path, caplog):
    from test_gpu_annotate import _clip_and_table, _expected
    from ysmr_amd import annotate_video
    from ysmr_amd.helper_file import default_settings
    clip, df, per_frame = _clip_and_table()
    path = str(tmp_path / "clip.npy")
    np.save(path, clip)
    out = str(tmp_path / "results")
    s = default_settings(**{"log to file": False, "hip frames per batch": 5, "frames per second": 25.0, "log_level": logging.INFO,
                            "save video file extension": ".avi", "save video fourcc codec": "MJPG"})
    with caplog.at_level(logging.INFO, logger="ysmr"):
        written = annotate_video(path, df, settings=s, result_folder=out)      # three batches: 5, 5 and 2 frames
    assert written == os.path.join(out, "clip_annotated_output.avi") and os.path.isfile(written)
    assert "no encoder" not in caplog.text and "Motion-JPEG, quality 90" in caplog.text
    want = _expected(clip, per_frame)
    model = [jm.encode(f, 90) for f in want]
    got = _payloads(written)
    assert len(got) == 12
    for i in range(12):
        assert got[i] == model[i], "frame {}".format(i)
    assert (want != am.to_bgr(clip)).any()

    written2 = annotate_video(path, df, settings=s, result_folder=out, select_subtype=2)
    assert written2 == os.path.join(out, "motile_subtype_clip_annotated_output.avi")
    want_motile = _expected(clip, per_frame, subtype=2)
    assert _payloads(written2) == [jm.encode(f, 90) for f in want_motile] and (want_motile != want).any()
    assert sorted(os.listdir(out)) == ["clip_annotated_output.avi", "motile_subtype_clip_annotated_output.avi"]

    pytest.importorskip("PIL")
    from ysmr_amd.frames import AviVideo
    video = AviVideo(written)
    assert (video.frame_count, video.frames_available, video.height, video.width) == (12, 12, 48, 64)
    assert video.fps == 25.0
    frames = video.read(0, 12)
    video.close()
    for i in range(12):           # equal bytes decode equally: the reader's frames are Pillow's decode of the model's stream
        assert np.array_equal(np.asarray(frames[i]).reshape(48, 64, 3), _decode(model[i])), "frame {}".format(i)


def test_a_batch_larger_than_its_raw_size_is_encoded_again(tmp_path, caplog):
    import pandas as pd
    from ysmr_amd import annotate_video
    from ysmr_amd.helper_file import default_settings
    clip = np.random.default_rng(3).integers(0, 256, (7, 24, 40, 3), dtype=np.uint8)
    model = [jm.encode(f, 100) for f in clip]
    assert sum(len(jm.chunk(j)) for j in model[:5]) > 5 * 24 * 120            # the first batch does not fit its default buffer
    from avi_tools import write_avi
    path = str(tmp_path / "noise.avi")
    write_avi(path, clip, bits=24, fps=(25, 1))
    df = pd.DataFrame({"TRACK_ID": np.array([], np.int64), "POSITION_T": np.array([], np.int64), "POSITION_X": np.array([], np.float64),
                       "POSITION_Y": np.array([], np.float64), "moving": np.array([], np.int8), "turn_points": np.array([], np.int8),
                       "motility_phenotype": np.array([], np.int8)})
    s = default_settings(**{"log to file": False, "hip frames per batch": 5, "frames per second": 25.0, "hip video jpeg quality": 100,
                            "save video file extension": ".avi", "save video fourcc codec": "mjpg", "log_level": logging.DEBUG})
    with caplog.at_level(logging.DEBUG, logger="ysmr"):
        written = annotate_video(path, df, settings=s, result_folder=str(tmp_path / "results"))
    assert written is not None and "encoding them again" in caplog.text
    assert _payloads(written) == model
