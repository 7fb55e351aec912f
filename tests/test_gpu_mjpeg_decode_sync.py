"""GPU: ``ysmr_mjpeg_decode_batch_sync`` (csrc/mjpeg_decode.hip: k_mjd_destuff, k_mjd_sync, k_mjd_dc beside the kernels of
``ysmr_mjpeg_decode_batch``) against the NumPy model of the pixels (tests/jpeg_decode_model.py), byte for byte and status for
status: the fixture's streams, streams built to cross the boundaries ``ysmr_mjpeg_decode_sync_geometry`` reports, damaged
streams between good ones, restart-marked and restart-less frames in one call; then ``DeviceFrameFeed`` and ``track_bacteria``
with 'hip decode mjpeg' = 'always'."""
import ctypes
import functools
import os

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_model as jm
import mjpeg_sync_streams as ms
from test_gpu_mjpeg_decode import GUARD, _avi, _feed_frames, _mixed_444, _pixels, _settings, entry_of, stream_of
from test_mjpeg_decode_cpu import modelled, names

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def geometry():
    from ysmr_amd import _lib
    sub, per_pass = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.lib().ysmr_mjpeg_decode_sync_geometry(ctypes.byref(sub), ctypes.byref(per_pass))
    assert sub.value > 0 and per_pass.value > 0
    return sub.value, per_pass.value


@functools.lru_cache(maxsize=None)
def model(stream, height, width, sampling):
    status, pixels = dm.decode(stream, height, width, sampling)
    pixels.setflags(write=False)
    return status, pixels


def decode_sync(streams, height, width, sampling, fill=0xEE, max_chunk=None):
    """(status int32 [n], frames u8 [n, H, W(, 3)]) of one call of the new entry: the workspace pre-filled with ``fill``, the
    frames with 0xAA between two guards of 0xAA that must come back whole; pad bytes between the chunks as an AVI has them."""
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    n, channels = len(streams), 1 if sampling == 0 else 3
    padded = [s + bytes(len(s) & 1) for s in streams]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in padded])]).astype(np.int64)
    chunks = torch.from_numpy(np.frombuffer(b"".join(padded), np.uint8).copy()).cuda()
    offsets_dev = torch.from_numpy(offsets).cuda()
    if max_chunk is None:
        max_chunk = max(len(s) for s in padded)
    ws_bytes = L.ysmr_mjpeg_decode_sync_workspace_bytes(n, height, width, channels, sampling, max_chunk)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device="cuda")
    frame_bytes = height * width * channels
    out = torch.full((2 * GUARD + n * frame_bytes,), 0xAA, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.ysmr_mjpeg_decode_batch_sync(None, chunks.data_ptr(), offsets_dev.data_ptr(), n, height, width, channels, sampling,
                                              max_chunk, ws.data_ptr(), ws_bytes, out.data_ptr() + GUARD, status.data_ptr()),
               "ysmr_mjpeg_decode_batch_sync")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == 0xAA).all() and (got[-GUARD:] == 0xAA).all(), "a guard of frames_dev was written"
    shape = (n, height, width) if sampling == 0 else (n, height, width, 3)
    return status.cpu().numpy(), got[GUARD:-GUARD].reshape(shape)


def check_against_model(streams, height, width, sampling, **kw):
    status, frames = decode_sync(streams, height, width, sampling, **kw)
    for k, stream in enumerate(streams):
        want_status, want = model(stream, height, width, sampling)
        assert status[k] == want_status, "frame {}: status {} instead of {}".format(k, status[k], want_status)
        if want_status == 0:
            np.testing.assert_array_equal(frames[k], want, err_msg="frame {}".format(k))
    return status, frames


# ---- 1: the fixture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names())
def test_every_fixture_stream_equals_the_model(name):
    """With and without restart markers, supported or flagged; one frame per call, so that the guard lies directly behind the
    slot of a flagged frame."""
    e = entry_of(name)
    status, frames = decode_sync([stream_of(name)], e["height"], e["width"], e["sampling"])
    want_status, want = modelled(name)
    assert status[0] == want_status == e["status"]
    if want_status == 0:
        np.testing.assert_array_equal(frames[0], want)


# ---- 2: streams built to cross the boundaries --------------------------------------------------------------------------------------
def _noise_420_with(at_least):
    """A 4:2:0 noise frame of odd size with more than ``at_least`` subsequences: about 13 bytes of entropy data a block, six
    blocks an MCU of 16 x 16; the count is asserted by the caller."""
    sub, _ = geometry()
    side = int(np.ceil(np.sqrt(at_least * sub / 70.0)))
    return ms.noise(16 * side - 3, 16 * side - 5, 3)


def test_the_true_state_is_carried_from_pass_to_pass():
    sub, per_pass = geometry()
    stream, h, w, s = _noise_420_with(per_pass + 1)
    assert ms.subsequences(stream, sub) > per_pass + 1 and h % 2 == 1 and w % 2 == 1
    status, _ = check_against_model([stream], h, w, s)
    assert status[0] == 0


def test_a_pass_wider_than_a_wave():
    sub, per_pass = geometry()
    if per_pass <= 66:
        pytest.skip("a pass is no wider than a wave")
    stream, h, w, s = _noise_420_with(65)
    assert 64 < ms.subsequences(stream, sub) < per_pass
    status, _ = check_against_model([stream], h, w, s)
    assert status[0] == 0


def test_the_all_zero_frame_over_two_passes():
    """Six bits per block, the same for ever: no lane that starts off the code's boundaries finds them; the true state walks
    through the pass a lane per round."""
    sub, per_pass = geometry()
    side = int(np.ceil(np.sqrt(per_pass * sub * 8 / 6.0))) + 1
    stream, h, w, s = ms.zeros(side, side + 1)
    assert ms.subsequences(stream, sub) > per_pass
    status, _ = check_against_model([stream], h, w, s)
    assert status[0] == 0


def test_long_symbols_and_stuffed_bytes():
    sub, _ = geometry()
    stream, h, w, s = ms.dense()
    assert stream.count(b"\xff\x00") >= 50 and ms.subsequences(stream, sub) >= 3
    status, _ = check_against_model([stream], h, w, s)
    assert status[0] == 0


def test_the_dc_prediction_passes_16_bits():
    stream, h, w, s = ms.dc_wrap()
    status, _ = check_against_model([stream], h, w, s)
    assert status[0] == 0


@pytest.mark.parametrize("sampling", (0, 1, 2))
def test_the_dc_sums_follow_the_scan(sampling):
    """Gray, 4:4:4 and 4:2:2 (4:2:0 is the case above): odd sizes, at least three subsequences."""
    sub, _ = geometry()
    stream, h, w, s = ms.noise(53, 75, sampling)
    assert ms.subsequences(stream, sub) >= 3
    status, _ = check_against_model([stream], h, w, s)
    assert status[0] == 0


# ---- 3: damaged streams between two good frames ------------------------------------------------------------------------------------
def _raw_position(stream, k):
    """Where byte k of the entropy data WITHOUT its stuffing lies in the stream."""
    at = stream.index(b"\xff\xda")
    at += 2 + int.from_bytes(stream[at + 2:at + 4], "big")
    for _ in range(k):
        at += 2 if stream[at] == 0xFF else 1
    return at


def _between_good_frames(damaged, expect=None, **kw):
    """[good, damaged, good] in one call: the good frames come back as they are alone; the damaged one gets ``expect`` (None:
    the model's status), and the model's pixels where that is 0.  Returns the status."""
    good, h, w, s = ms.noise(61, 75, 3)
    other = ms.noise(61, 75, 3, seed=6)[0]
    status, frames = decode_sync([good, damaged, other], h, w, s, **kw)
    want, pixels = model(damaged, h, w, s)
    if expect is None:
        expect = want
    assert list(status) == [0, expect, 0]
    np.testing.assert_array_equal(frames[0], model(good, h, w, s)[1])
    np.testing.assert_array_equal(frames[2], model(other, h, w, s)[1])
    if expect == 0:
        np.testing.assert_array_equal(frames[1], pixels)
    return expect


def test_truncated_frames():
    sub, _ = geometry()
    good = ms.noise(61, 75, 3)[0]
    count = ms.subsequences(good, sub)
    assert count >= 4
    for k in (sub + 1, 2 * sub, (count - 1) * sub + 1):     # one byte into the second subsequence, at a boundary, in the last one
        cut = good[:_raw_position(good, k)]
        assert model(cut, 61, 75, 3)[0] == dm.CORRUPT
        _between_good_frames(cut)


def test_markers_inside_the_entropy_data():
    good = ms.noise(61, 75, 3)[0]
    middle = _raw_position(good, ms.entropy_bytes(good) // 2)
    for marker in (b"\xff\xd9", b"\xff\xd0"):                             # the data ends there; an RSTn in a frame without DRI
        spliced = good[:middle] + marker + good[middle:]
        assert model(spliced, 61, 75, 3)[0] == dm.CORRUPT
        _between_good_frames(spliced)


def test_overwritten_bytes():
    """The model decides whether the frame survives; the device agrees, and where it does the pixels are the model's."""
    good = ms.noise(61, 75, 3)[0]
    rng = np.random.default_rng(21)
    seen = set()
    for k in rng.integers(0, ms.entropy_bytes(good), 5):
        at = _raw_position(good, int(k))
        seen.add(_between_good_frames(good[:at] + bytes([good[at] ^ 0x5A]) + good[at + 1:]))
    assert seen <= {0, dm.CORRUPT}


def test_a_chunk_longer_than_max_chunk_bytes():
    good = ms.noise(61, 75, 3)[0]
    longer = good + bytes(64)                                               # (bytes behind EOI are ignored: the model's status is 0)
    assert model(longer, 61, 75, 3)[0] == 0
    bound = max(len(good), len(ms.noise(61, 75, 3, seed=6)[0])) + 2         # holds both good frames of the call and their pad bytes
    assert bound < len(longer)
    _between_good_frames(longer, dm.CORRUPT, max_chunk=bound)
    _between_good_frames(longer, 0, max_chunk=len(longer))


# ---- 4, 5: one call of many frames; hygiene ------------------------------------------------------------------------------------------
def _mixed_65():
    mixed = _mixed_444()                                                    # two without restart markers, one with a restart interval per MCU row
    noise = np.random.default_rng(10).integers(0, 256, (23, 41, 3), dtype=np.uint8)
    kinds = mixed + [jm.encode(noise, 50), ms.noise(23, 41, 1)[0]]
    streams = [kinds[k % 5] for k in range(65)]
    streams[37] = stream_of("444_cut_in_half_23x41")
    return streams


def test_restart_marked_and_restartless_frames_in_one_call():
    streams = _mixed_65()
    assert sum(b"\xff\xdd" in s for s in streams) >= 20 and sum(b"\xff\xdd" not in s for s in streams) >= 20
    status, _ = check_against_model(streams, 23, 41, 1)
    assert [k for k in range(65) if status[k]] == [37] and status[37] == dm.CORRUPT


def test_nothing_found_in_the_workspace_is_used():
    streams = _mixed_65()[:9] + [ms.noise(23, 41, 1, seed=12)[0]]
    a = decode_sync(streams, 23, 41, 1, fill=0xEE)
    b = decode_sync(streams, 23, 41, 1, fill=0x11)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert not a[0].any()


def test_arguments():
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert L.ysmr_mjpeg_decode_batch_sync(None, p, p, 1, 8, 8, 3, 4, 100, p, 4096, p, p) == _lib.YSMR_ERR_ARG
    assert L.ysmr_mjpeg_decode_batch_sync(None, p, p, 1, 8, 8, 1, 0, 0, p, 4096, p, p) == _lib.YSMR_ERR_ARG
    assert b"max_chunk_bytes" in L.ysmr_last_error()
    assert L.ysmr_mjpeg_decode_batch_sync(None, p, p, 1, 64, 64, 3, 1, 100, p, 4096, p, p) == _lib.YSMR_ERR_ARG
    assert b"workspace" in L.ysmr_last_error()
    assert L.ysmr_mjpeg_decode_batch_sync(None, p, None, 1, 8, 8, 1, 0, 100, p, 4096, p, p) == _lib.YSMR_ERR_ARG


# ---- 6: through DeviceFrameFeed --------------------------------------------------------------------------------------------------------
class _Spy:
    """The library's handle, recording which entry points were asked for."""

    def __init__(self, real):
        self._real, self.asked = real, []

    def __getattr__(self, name):
        self.asked.append(name)
        return getattr(self._real, name)


def test_the_feed_decodes_restartless_frames_on_the_device(tmp_path, monkeypatch):
    from ysmr_amd import _lib
    from ysmr_amd.frames import AviVideo
    a = "422_more_31x33_q100_noise"
    order = [n for n in names(supported=True) if n.startswith("422_") and entry_of(n)["height"] == 31 and b"\xff\xdd" not in stream_of(n)]
    assert a in order
    order = [order[k % len(order)] for k in range(7)]                       # batches of 3, 3 and 1
    video = AviVideo(_avi(tmp_path / "m.avi", order, 31, 33))
    assert video.jpeg_layout is None and video.jpeg_layout_for(3, needs_restart=False)[0] == 2
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    host = []

    def no_host(self, blob, dst):
        raise AssertionError("the host decoded a frame")

    def recording_host(self, blob, dst):
        dst[...] = _pixels(next(n for n in order if stream_of(n) == blob.getvalue()))
        host.append(1)

    monkeypatch.setattr(AviVideo, "_decode_jpeg", no_host)
    got = _feed_frames(video, 3, decode_on_device="always")
    assert got.shape == (7, 31, 33, 3)
    for k, name in enumerate(order):
        np.testing.assert_array_equal(got[k], _pixels(name), err_msg="frame {}".format(k))
    assert "ysmr_mjpeg_decode_batch_sync" in spy.asked and "ysmr_mjpeg_decode_sync_workspace_bytes" in spy.asked
    assert "ysmr_mjpeg_decode_batch" not in spy.asked
    # True: the same file is the host's, as before
    del spy.asked[:]
    monkeypatch.setattr(AviVideo, "_decode_jpeg", recording_host)
    got = _feed_frames(video, 3, decode_on_device=True)
    video.close()
    assert len(host) == 7 and got.shape == (7, 31, 33, 3)
    for k, name in enumerate(order):
        np.testing.assert_array_equal(got[k], _pixels(name), err_msg="frame {}".format(k))
    assert not [n for n in spy.asked if n.startswith("ysmr_mjpeg_decode")]


# ---- 7: end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restartless_clip():
    """32 frames of a small synthetic clip as gray JPEGs WITHOUT restart markers: the encoder model's quantised luminance
    coefficients, written by ``build_stream``."""
    from ysmr_amd.synth import SyntheticVideo
    frames = SyntheticVideo(96, 128, 8, seed=4).frames(32)
    table = jm.quant_tables(75)[0][jm.ZIGZAG]
    blobs = []
    for f in frames:
        coef = jm.coefficients(np.repeat(f[..., None], 3, axis=2), 75)
        blobs.append(ms.gen().build_stream(96, 128, 0, [coef[:, :, 0, :]], [table]))
    return frames, blobs


def test_track_bacteria_from_a_restartless_motion_jpeg_avi(tmp_path):
    """'hip decode mjpeg' = 'always' (the device) and False (the host path) write the same ``_list.csv`` bytes."""
    from avi_tools import write_avi
    from ysmr_amd.frames import AviVideo
    from ysmr_amd.track_eval import track_bacteria
    frames, blobs = _restartless_clip()
    assert not any(b"\xff\xdd" in b for b in blobs)
    written = {}
    for sub, mode in (("d", "always"), ("h", False)):
        os.makedirs(tmp_path / sub)
        path = str(tmp_path / sub / "clip.avi")
        write_avi(path, frames, 24, fps=(30, 1), jpeg=blobs)
        video = AviVideo(path)
        assert video.jpeg_layout is None and video.jpeg_layout_for(16, needs_restart=False)[0] == 0 and video.channels == 1
        video.close()
        res = track_bacteria(path, settings=_settings(**{"hip decode mjpeg": mode, "minimal frame count": 32}),
                             result_folder=str(tmp_path / sub), batch=16)
        assert res is not None and len(res[0]) > 50
        written[sub] = open(res[4], "rb").read()
    assert written["d"] == written["h"]
