"""GPU: ``ysmr_mjpeg_decode_batch`` (csrc/mjpeg_decode.hip) against its NumPy model (tests/jpeg_decode_model.py), byte for byte
and status for status; the Motion-JPEG staging mode of ``DeviceFrameFeed``; ``track_bacteria`` and ``annotate_video`` from a
Motion-JPEG AVI.  The streams come from tests/golden/mjpeg_decode_streams.npz and from the encoder's model: no Pillow is
needed (where the host path is the yardstick, what it raises without Pillow is the yardstick too)."""
import functools
import os

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_model as jm
from test_mjpeg_decode_cpu import fixture, modelled, names

pytestmark = pytest.mark.gpu

GUARD = 64


def stream_of(name):
    return next(s for e, s, _ in fixture() if e["name"] == name)


def entry_of(name):
    return next(e for e, _, _ in fixture() if e["name"] == name)


def decode_batch(streams, height, width, sampling):
    """(status int32 [n], frames u8 [n, H, W(, 3)]) of one call: the workspace pre-filled with 0xEE, the frames with 0xAA
    between two guards of 0xAA that must come back whole; pad bytes between the chunks as an AVI has them."""
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    n, channels = len(streams), 1 if sampling == 0 else 3
    padded = [s + bytes(len(s) & 1) for s in streams]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in padded])]).astype(np.int64)
    chunks = torch.from_numpy(np.frombuffer(b"".join(padded), np.uint8).copy()).cuda()
    offsets_dev = torch.from_numpy(offsets).cuda()
    ws_bytes = L.ysmr_mjpeg_decode_workspace_bytes(n, height, width, channels, sampling)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    frame_bytes = height * width * channels
    out = torch.full((2 * GUARD + n * frame_bytes,), 0xAA, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.ysmr_mjpeg_decode_batch(None, chunks.data_ptr(), offsets_dev.data_ptr(), n, height, width, channels, sampling,
                                         ws.data_ptr(), ws_bytes, out.data_ptr() + GUARD, status.data_ptr()), "ysmr_mjpeg_decode_batch")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == 0xAA).all() and (got[-GUARD:] == 0xAA).all(), "a guard of frames_dev was written"
    shape = (n, height, width) if sampling == 0 else (n, height, width, 3)
    return status.cpu().numpy(), got[GUARD:-GUARD].reshape(shape)


def check_against_model(streams, height, width, sampling):
    status, frames = decode_batch(streams, height, width, sampling)
    seen = {}
    for k, stream in enumerate(streams):
        if stream not in seen:
            seen[stream] = dm.decode(stream, height, width, sampling)
        want_status, want = seen[stream]
        assert status[k] == want_status, "frame {}: status {} instead of {}".format(k, status[k], want_status)
        if want_status == 0:
            np.testing.assert_array_equal(frames[k], want, err_msg="frame {}".format(k))
    return status, frames


@pytest.mark.parametrize("name", names())
def test_every_fixture_stream_equals_the_model(name):
    """One frame per call, so that the guard lies directly behind the slot of a flagged frame."""
    e = entry_of(name)
    status, frames = decode_batch([stream_of(name)], e["height"], e["width"], e["sampling"])
    want_status, want = modelled(name)
    assert status[0] == want_status == e["status"]
    if want_status == 0:
        np.testing.assert_array_equal(frames[0], want)


def test_the_encoders_streams_equal_the_model():
    import test_mjpeg_cpu
    for name, bgr in test_mjpeg_cpu.images().items():
        streams = [test_mjpeg_cpu.encoded(name, q)[0] for q in test_mjpeg_cpu.QUALITIES]
        status, _ = check_against_model(streams, bgr.shape[0], bgr.shape[1], 1)
        assert not status.any()


def _mixed_444():
    """Three 23 x 41 streams with different quantisation and Huffman tables (Pillow's optimised ones, Pillow's standard
    ones at another quality, the encoder model's with one restart interval per MCU row)."""
    noise = np.random.default_rng(9).integers(0, 256, (23, 41, 3), dtype=np.uint8)
    return [stream_of("444_optimize_23x41_q100_saturated"), stream_of("444_more_23x41_q50_flat"), jm.encode(noise, 90)]


def test_one_batch_with_different_tables_and_a_damaged_frame():
    mixed = _mixed_444()
    status, frames = check_against_model(mixed, 23, 41, 1)
    assert not status.any()
    # good / cut in half / good: the good frames are what they were, the middle one is flagged
    cut = stream_of("444_cut_in_half_23x41")
    status, again = check_against_model([mixed[0], cut, mixed[2]], 23, 41, 1)
    assert list(status) == [0, dm.CORRUPT, 0]
    np.testing.assert_array_equal(again[0], frames[0])
    np.testing.assert_array_equal(again[2], frames[2])
    # every kind of flagged frame between good ones
    for name in names(supported=False):
        if entry_of(name)["sampling"] == 1:
            status, again = decode_batch([mixed[1], stream_of(name), mixed[0]], 23, 41, 1)
            assert list(status) == [0, entry_of(name)["status"], 0], name
            np.testing.assert_array_equal(again[0], frames[1])
            np.testing.assert_array_equal(again[2], frames[0])


@pytest.mark.parametrize("n", [1, 8, 65])
def test_batch_sizes(n):
    """The same stream eight times gives eight identical frames; 65 frames are more than a wave of the header kernel."""
    mixed = _mixed_444()
    streams = [mixed[2]] * n if n == 8 else [mixed[k % 3] for k in range(n)]
    status, frames = decode_batch(streams, 23, 41, 1)
    assert not status.any()
    want = [dm.decode(s, 23, 41, 1)[1] for s in mixed]
    for k in range(n):
        np.testing.assert_array_equal(frames[k], want[2 if n == 8 else k % 3], err_msg="frame {}".format(k))


def test_more_intervals_than_the_entropy_grid_takes_at_once():
    """16424 x 9 from the encoder's model: 2053 restart intervals of two MCUs, more than the 32 workgroups of 64 lanes
    that a frame gets at most -- the kernel's loop over the intervals runs a second time for five of them."""
    tall = np.random.default_rng(3).integers(0, 256, (16424, 9, 3), dtype=np.uint8)
    tall[4000:9000] = 128                                                   # (flat blocks: short intervals beside long ones)
    stream = jm.encode(tall, 50)
    status, _ = check_against_model([stream, stream], 16424, 9, 1)
    assert not status.any()


def test_arguments():
    from ysmr_amd import _lib
    L = _lib.lib()
    assert L.ysmr_mjpeg_decode_workspace_bytes(1, 8, 8, 3, 4) == 0 and L.ysmr_mjpeg_decode_workspace_bytes(1, 8, 8, 3, -1) == 0
    assert L.ysmr_mjpeg_decode_workspace_bytes(1, 8, 8, 3, 0) == 0 and L.ysmr_mjpeg_decode_workspace_bytes(1, 8, 8, 1, 2) == 0
    assert L.ysmr_mjpeg_decode_workspace_bytes(0, 8, 8, 1, 0) == 0 and L.ysmr_mjpeg_decode_workspace_bytes(1, 8, 8, 1, 0) > 0
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ERR_ARG = _lib.YSMR_ERR_ARG
    assert L.ysmr_mjpeg_decode_batch(None, buf.data_ptr(), buf.data_ptr(), 1, 8, 8, 3, 4, buf.data_ptr(), 4096, buf.data_ptr(),
                                     buf.data_ptr()) == ERR_ARG
    assert L.ysmr_mjpeg_decode_batch(None, buf.data_ptr(), buf.data_ptr(), 1, 64, 64, 3, 1, buf.data_ptr(), 4096, buf.data_ptr(),
                                     buf.data_ptr()) == ERR_ARG                                # workspace too small
    assert b"workspace" in L.ysmr_last_error()


# ---- through DeviceFrameFeed ---------------------------------------------------------------------------------------------------
def _avi(path, stream_names, h, w):
    from avi_tools import write_avi
    blobs = [stream_of(n) for n in stream_names]
    write_avi(str(path), np.zeros((len(blobs), h, w), np.uint8), 24, fps=(25, 1), jpeg=blobs)
    return str(path)


def _feed_frames(video, batch, **kw):
    import torch
    from ysmr_amd.frames import DeviceFrameFeed
    feed = DeviceFrameFeed(video, batch, "cuda:0", readers=3, near_gpu=False, **kw)
    out = []
    try:
        for frames_dev, f0, n, slot in feed:
            assert f0 == len(out)
            out.extend(frames_dev.cpu().numpy())
            ev = torch.cuda.Event()
            ev.record()
            feed.release(slot, ev)
    finally:
        feed.close()
    return np.stack(out)


def _pixels(name):
    return next(p for e, _, p in fixture() if e["name"] == name)


def test_the_feed_delivers_the_fixtures_pixels_without_the_host(tmp_path, monkeypatch):
    from ysmr_amd.frames import AviVideo
    a, b = "422_rows_31x33_q100_flat", "422_more_31x33_q100_noise"          # the first frame has a restart interval
    order = [a, b, b, a, b, a, a]                                           # batches of 3, 3 and 1; odd- and even-sized chunks
    video = AviVideo(_avi(tmp_path / "m.avi", order, 31, 33))
    assert video.jpeg_layout is not None and video.jpeg_layout[0] == 2

    def no_host(self, blob, dst):
        raise AssertionError("the host decoded a frame")

    monkeypatch.setattr(AviVideo, "_decode_jpeg", no_host)
    got = _feed_frames(video, 3)
    video.close()
    assert got.shape == (7, 31, 33, 3)
    for k, name in enumerate(order):
        np.testing.assert_array_equal(got[k], _pixels(name), err_msg="frame {}".format(k))
    # a file without restart intervals is the host's by default, and the device's where the feed is told 'always'
    order = ["L_more_23x41_q50_noise"] * 3
    video = AviVideo(_avi(tmp_path / "n.avi", order, 23, 41))
    assert video.jpeg_layout is None
    assert video.jpeg_layout_for(2, needs_restart=False)[0] == 0
    got = _feed_frames(video, 2, decode_on_device="always")
    video.close()
    assert got.shape == (3, 23, 41)
    for k in range(3):
        np.testing.assert_array_equal(got[k], _pixels(order[k]))


def _host_path(video, k):
    """What the host path makes of frame k: ('frame', pixels) or ('raises', type, text)."""
    try:
        return ("frame", video.read(k, 1)[0])
    except (OSError, ValueError) as exc:
        return ("raises", type(exc), str(exc))


def _with_restarts_first(tmp_path, rest):
    """A 23 x 41 4:4:4 file whose first frame comes from the encoder's model (one restart interval per MCU row)."""
    from avi_tools import write_avi
    first = _mixed_444()[2]
    write_avi(str(tmp_path / "m.avi"), np.zeros((1 + len(rest), 23, 41), np.uint8), 24, fps=(25, 1), jpeg=[first] + [stream_of(n) for n in rest])
    return str(tmp_path / "m.avi"), dm.decode(first, 23, 41, 1)[1]


@pytest.mark.parametrize("flagged", ["444_cut_in_half_23x41", "444_progressive_23x41", "444_app14_23x41"])
def test_the_feed_sends_flagged_frames_to_the_host_path(tmp_path, flagged):
    """A frame the device flags is decoded by the host path: a truncated one raises what it raises there (Pillow's OSError;
    the reader's ValueError where Pillow is absent), a progressive one arrives as Pillow decodes it."""
    from ysmr_amd.frames import AviVideo
    a, b = "444_optimize_23x41_q100_saturated", "444_more_23x41_q50_flat"
    order = [a, b, a, flagged, a]
    path, first = _with_restarts_first(tmp_path, order)
    video = AviVideo(path)
    assert video.jpeg_layout is not None
    host = _host_path(video, 4)
    try:
        if host[0] == "raises":
            with pytest.raises(host[1]) as caught:
                _feed_frames(video, 4)
            assert str(caught.value) == host[2]
        else:
            got = _feed_frames(video, 4)
            np.testing.assert_array_equal(got[4], host[1])
            np.testing.assert_array_equal(got[0], first)
            for k in (1, 2, 3, 5):
                np.testing.assert_array_equal(got[k], modelled(order[k - 1])[1])
    finally:
        video.close()


def test_the_feed_without_device_decode_is_the_host_path(tmp_path):
    from ysmr_amd.frames import AviVideo
    a, b = "444_optimize_23x41_q100_saturated", "444_more_23x41_q50_flat"
    path, first = _with_restarts_first(tmp_path, [a, b])
    video = AviVideo(path)
    assert video.jpeg_layout is not None
    host = _host_path(video, 0)
    try:
        if host[0] == "raises":
            with pytest.raises(host[1]):
                _feed_frames(video, 2, decode_on_device=False)
        else:
            got = _feed_frames(video, 2, decode_on_device=False)
            np.testing.assert_array_equal(got, video.read(0, 3))
            np.testing.assert_array_equal(got[0], first)
            np.testing.assert_array_equal(got[2], modelled(b)[1])
    finally:
        video.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip():
    """(JPEGs of a small synthetic clip, gray replicated to B, G, R; the frames the model decodes from them), made once."""
    from ysmr_amd.synth import SyntheticVideo
    frames = SyntheticVideo(96, 128, 8, seed=4).frames(40)
    blobs = [jm.encode(np.repeat(f[..., None], 3, axis=2), 75) for f in frames]
    decoded = np.stack([dm.decode(b, 96, 128, 1)[1] for b in blobs])
    decoded.setflags(write=False)
    return blobs, decoded


def _settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False,
                            "log to file": False, "minimal frame count": 40})
    s.update(kw)
    return s


def test_track_bacteria_from_a_motion_jpeg_avi(tmp_path):
    """The same csv bytes from the Motion-JPEG AVI as from the uncompressed AVI of the frames the model decodes."""
    from avi_tools import write_avi
    from ysmr_amd.frames import AviVideo
    from ysmr_amd.track_eval import track_bacteria
    blobs, decoded = _clip()
    for sub in ("m", "u"):
        os.makedirs(tmp_path / sub)
    write_avi(str(tmp_path / "m" / "clip.avi"), decoded[..., 0], 24, fps=(30, 1), jpeg=blobs)
    write_avi(str(tmp_path / "u" / "clip.avi"), decoded, 24, fps=(30, 1))
    video = AviVideo(str(tmp_path / "m" / "clip.avi"))
    assert video.jpeg_layout is not None and video.jpeg_layout[0] == 1 and video.channels == 3
    video.close()
    rm = track_bacteria(str(tmp_path / "m" / "clip.avi"), settings=_settings(), result_folder=str(tmp_path / "m"), batch=16)
    ru = track_bacteria(str(tmp_path / "u" / "clip.avi"), settings=_settings(), result_folder=str(tmp_path / "u"), batch=16)
    assert rm is not None and ru is not None and rm[1:4] == ru[1:4] == (30.0, 96, 128)
    assert len(rm[0]) > 100 and rm[0].equals(ru[0])
    assert open(rm[4], "rb").read() == open(ru[4], "rb").read()


def test_annotate_video_reads_a_motion_jpeg_avi(tmp_path):
    import pandas as pd
    from avi_tools import write_avi
    from ysmr_amd import annotate_video
    blobs, decoded = _clip()
    rows = [(7, t, 20.0 + t, 30.0 + 0.5 * t, 1, 0, 2) for t in range(12)] + [(9, t, 90.0 - t, 60.0, 0, 0, 0) for t in range(3, 12)]
    df = pd.DataFrame(rows, columns=["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "moving", "turn_points", "motility_phenotype"])
    df = df.astype({"TRACK_ID": np.int64, "POSITION_T": np.int64, "moving": np.int8, "turn_points": np.int8, "motility_phenotype": np.int8})
    written = {}
    for sub in ("m", "u"):
        os.makedirs(tmp_path / sub)
        path = str(tmp_path / sub / "clip.avi")
        if sub == "m":
            write_avi(path, decoded[:12, ..., 0], 24, fps=(25, 1), jpeg=blobs[:12])
        else:
            write_avi(path, decoded[:12], 24, fps=(25, 1))
        s = _settings(**{"hip frames per batch": 5, "frames per second": 25.0})
        written[sub] = annotate_video(path, df, settings=s, result_folder=str(tmp_path / sub / "out"))
        assert written[sub] is not None and os.path.isfile(written[sub])
    assert open(written["m"], "rb").read() == open(written["u"], "rb").read()
