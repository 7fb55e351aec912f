"""GPU: ``ysmr_tiff_decode_batch`` (csrc/tiff_decode.hip) against its model (tests/tiff_decode_model.py), byte for byte and status
for status; the TIFF staging mode of ``DeviceFrameFeed``; ``track_bacteria`` and ``annotate_video`` from a TIFF stack.  The files
come from tests/golden/tiff_decode_streams.npz, from the minimal writer (tests/tiff_tools.py) and from the model's LZW encoder:
no Pillow is needed (where the host path is the yardstick, what it raises without Pillow is the yardstick too)."""
import functools
import os
import sys

import numpy as np
import pytest

import tiff_decode_model as tm
import tiff_tools as tt
from test_tiff_cpu import bodies_of, entry, hand_built, names, opened

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = 0xAA


def decode_batch(frames_bodies, height, width, channels, compression, predictor=1, photometric=None, rows_per_strip=None):
    """(status int32 [n], frames u8 [n, H * W * channels], status per strip) of one call.  ``frames_bodies``: per frame the bodies
    of its strips.  Every body begins at an ODD offset behind a pad byte that no strip owns; the frames are pre-filled with 0xAA
    between two guards of 0xAA that must come back whole, the workspace with 0xEE."""
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    n = len(frames_bodies)
    photometric = (2 if channels == 3 else 1) if photometric is None else photometric
    rows_per_strip = height if rows_per_strip is None else rows_per_strip
    blob, table = bytearray(), []
    for f, bodies in enumerate(frames_bodies):
        assert len(bodies) == -(-height // rows_per_strip)
        for s, body in enumerate(bodies):
            blob += b"\x5A" * (1 if len(blob) % 2 == 0 else 2)
            table.append((f, s * rows_per_strip, min(rows_per_strip, height - s * rows_per_strip), len(blob), len(body)))
            blob += body
    blob += b"\x5A"
    bodies_dev = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda()
    strips_dev = torch.from_numpy(np.array(table, np.int32)).cuda()
    ws_bytes = L.ysmr_tiff_decode_workspace_bytes(n, height, width, channels, compression, predictor, photometric, rows_per_strip, len(blob))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    frame_bytes = height * width * channels
    out = torch.full((2 * GUARD + n * frame_bytes,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.ysmr_tiff_decode_batch(None, bodies_dev.data_ptr(), strips_dev.data_ptr(), len(table), n, height, width, channels,
                                        compression, predictor, photometric, ws.data_ptr(), ws_bytes, out.data_ptr() + GUARD,
                                        status.data_ptr()), "ysmr_tiff_decode_batch")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[-GUARD:] == CANARY).all(), "a guard of frames_out was written"
    return status.cpu().numpy(), got[GUARD:-GUARD].reshape(n, frame_bytes), ws.cpu().numpy().view(np.int32)[:len(table)]


def file_batch(tmp_path, name):
    """Everything ``decode_batch`` needs of a recorded file, and its frames."""
    _, data, frames = entry(name)
    video = opened(tmp_path, data)
    args = dict(height=video.height, width=video.width, channels=video.channels, compression=video._compression,
                predictor=video._predictor, photometric=video._photometric, rows_per_strip=video._rows_per_strip)
    bodies = [bodies_of(video, data, k) for k in range(video.frame_count)]
    video.close()
    return bodies, args, frames


@pytest.mark.parametrize("name", names())
def test_every_recorded_file_equals_the_model(tmp_path, name):
    bodies, args, frames = file_batch(tmp_path, name)
    status, got, per_strip = decode_batch(bodies, **args)
    assert not status.any() and not per_strip.any()
    np.testing.assert_array_equal(got.reshape(frames.shape), frames)       # (the model equals them: test_tiff_cpu)


@pytest.mark.parametrize("case", hand_built(), ids=[c[0] for c in hand_built()])
def test_every_hand_built_stream_equals_the_model(case):
    """One strip, one frame: the status is the model's, the bytes the model wrote are there, and behind them nothing was written."""
    name, width, height, compression, body, want = case
    status, got, per_strip = decode_batch([[body]], height, width, 1, compression)
    want_status, data = tm.decode_strip(body, width * height, compression)
    assert want_status == want and status[0] == want and per_strip[0] == want
    assert bytes(got[0][:len(data)]) == data
    assert (got[0][len(data):] == CANARY).all()


def test_the_lzw_table_at_its_last_entry():
    """3839 data codes without a Clear fill the table to entry 4095 and decode; the 3840th has no entry to add and is flagged,
    with everything before it in place."""
    noise = np.random.default_rng(12).integers(0, 256, (96, 96), dtype=np.uint8).tobytes()
    full = tm.lzw_encode(noise, clear_after=tm.MAX_RUN + 1)
    over = tm.lzw_encode(noise, clear_after=1 << 30)
    assert tm.lzw_decode(full, len(noise)) == (0, noise)
    want_status, data = tm.lzw_decode(over, len(noise))
    assert want_status == tm.BAD_CODE and 3839 <= len(data) < len(noise)
    status, got, _ = decode_batch([[full], [over]], 96, 96, 1, 5)
    assert list(status) == [0, tm.BAD_CODE]
    assert bytes(got[0]) == noise and bytes(got[1][:len(data)]) == data and (got[1][len(data):] == CANARY).all()


@functools.lru_cache(maxsize=None)
def _stack():
    """The three pages of the recorded LZW stack: (bodies per frame, arguments, frames)."""
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        return file_batch(pathlib.Path(tmp), "lzw_stack_3x40x52")


@pytest.mark.parametrize("n", [1, 8, 65])
def test_batch_sizes(n):
    bodies, args, frames = _stack()
    status, got, _ = decode_batch([bodies[k % 3] for k in range(n)], **args)
    assert not status.any()
    for k in range(n):
        np.testing.assert_array_equal(got[k].reshape(40, 52), frames[k % 3], err_msg="frame {}".format(k))


@pytest.mark.parametrize("compression", [1, 5, 32773])
def test_more_strips_than_the_grid_takes_at_once(compression):
    """65 frames of 64 one-row strips are 4160 strips, more than the 4096 workgroups a launch gets: 64 of them take a second strip."""
    rng = np.random.default_rng(compression)
    rows = rng.integers(0, 256, (64, 5), dtype=np.uint8)                       # 64 different rows, shuffled per frame
    encoded = [r.tobytes() if compression == 1 else tm.lzw_literals(r.tobytes()) if compression == 5 else bytes([4]) + r.tobytes()
               for r in rows]
    order = [rng.permutation(64) for _ in range(65)]
    status, got, per_strip = decode_batch([[encoded[j] for j in order[f]] for f in range(65)], 64, 5, 1, compression, rows_per_strip=1)
    assert not status.any() and not per_strip.any() and len(per_strip) == 4160
    for f in range(65):
        np.testing.assert_array_equal(got[f].reshape(64, 5), rows[order[f]], err_msg="frame {}".format(f))


def test_a_damaged_frame_between_good_ones():
    bodies, args, frames = _stack()
    cut = [bodies[1][0], bodies[1][1][:len(bodies[1][1]) // 2], bodies[1][2]]
    status, got, per_strip = decode_batch([bodies[0], cut, bodies[2]], **args)
    assert list(status) == [0, tm.SHORT, 0] and list(per_strip) == [0, 0, 0, 0, tm.SHORT, 0, 0, 0, 0]
    np.testing.assert_array_equal(got[0].reshape(40, 52), frames[0])
    np.testing.assert_array_equal(got[2].reshape(40, 52), frames[2])
    # the damaged frame's sound strips are in place too, and its cut strip wrote what the model writes and no further
    damaged = got[1].reshape(40, 52)
    np.testing.assert_array_equal(damaged[:16], frames[1][:16])
    np.testing.assert_array_equal(damaged[32:], frames[1][32:])
    _, data = tm.lzw_decode(cut[1], 16 * 52)
    middle = damaged[16:32].reshape(-1)
    assert bytes(middle[:len(data)]) == data and (middle[len(data):] == CANARY).all()
    # every kind of flagged strip between good frames
    for name, width, height, compression, body, want in hand_built():
        if want and compression == 5 and (width, height) == (4, 2):
            good = tm.lzw_literals(bytes(range(8)))
            status, got, _ = decode_batch([[good], [body], [good]], 2, 4, 1, 5)
            assert list(status) == [0, want, 0], name
            assert bytes(got[0]) == bytes(got[2]) == bytes(range(8)), name


def test_a_strip_table_row_outside_the_frame_writes_nothing():
    """The kernels check every row of the table against the call's geometry before they touch memory."""
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    body = tm.lzw_literals(bytes(range(8)))
    blob = torch.from_numpy(np.frombuffer(body * 4, np.uint8).copy()).cuda()
    for bad in ((2, 0, 2), (0, 1, 2), (0, -1, 2), (-1, 0, 2), (0, 0, 0), (0, 0, 3)):
        table = torch.from_numpy(np.array([(0, 0, 2, 0, len(body)), bad + (len(body), len(body))], np.int32)).cuda()
        out = torch.full((2 * GUARD + 16,), CANARY, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
        for compression in (1, 5, 32773):
            _lib.check(L.ysmr_tiff_decode_batch(None, blob.data_ptr(), table.data_ptr(), 2, 2, 2, 4, 1, compression, 1,
                                                1, ws.data_ptr(), 256, out.data_ptr() + GUARD, status.data_ptr()), "ysmr_tiff_decode_batch")
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert ws.cpu().numpy().view(np.int32)[1] == tm.TABLE, bad
            assert (got[:GUARD] == CANARY).all() and (got[GUARD + 8:] == CANARY).all(), bad
            if 0 <= bad[0] < 2:
                assert status.cpu().numpy()[bad[0]] & tm.TABLE, bad


def test_refused_arguments_launch_nothing():
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    size = L.ysmr_tiff_decode_workspace_bytes
    assert size(1, 8, 8, 1, 5, 1, 1, 8, 100) > 0 and size(2, 8, 8, 3, 32773, 2, 2, 3, 0) > 0
    for refused in ((0, 8, 8, 1, 5, 1, 1, 8, 100), (1, 0, 8, 1, 5, 1, 1, 8, 100), (1, 8, -1, 1, 5, 1, 1, 8, 100), (1, 8, 8, 2, 5, 1, 1, 8, 100),
                    (1, 8, 8, 1, 8, 1, 1, 8, 100), (1, 8, 8, 1, 5, 3, 1, 8, 100), (1, 8, 8, 1, 5, 1, 2, 8, 100), (1, 8, 8, 3, 5, 1, 1, 8, 100),
                    (1, 8, 8, 1, 5, 1, 1, 0, 100), (1, 8, 8, 1, 5, 1, 1, 9, 100), (1, 8, 8, 1, 5, 1, 1, 8, -1), (1, 8, 8, 1, 5, 1, 1, 8, 1 << 31),
                    (1, 1 << 16, 1 << 15, 1, 5, 1, 1, 8, 100), ((1 << 31) - 1, 8, 8, 1, 5, 1, 1, 1, 100)):
        assert size(*refused) == 0, refused
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def call(n_strips=1, n_frames=1, height=8, width=8, channels=1, compression=5, predictor=1, photometric=1, ws_bytes=256, out=p):
        return L.ysmr_tiff_decode_batch(None, p, p, n_strips, n_frames, height, width, channels, compression, predictor, photometric, p,
                                        ws_bytes, out, p)

    assert call(n_strips=3, n_frames=2) == _lib.YSMR_ERR_ARG and b"tile" in L.ysmr_last_error()
    assert call(n_strips=6, height=10) == _lib.YSMR_ERR_ARG                # 10 rows in 6 strips: no such file
    assert call(n_strips=9) == _lib.YSMR_ERR_ARG                           # more strips than rows
    assert call(compression=8) == _lib.YSMR_ERR_ARG and b"compression" in L.ysmr_last_error()
    assert call(channels=3) == _lib.YSMR_ERR_ARG and call(photometric=2) == _lib.YSMR_ERR_ARG and call(predictor=0) == _lib.YSMR_ERR_ARG
    assert call(out=0) == _lib.YSMR_ERR_ARG and b"NULL" in L.ysmr_last_error()
    assert call(n_strips=8 * 80, n_frames=80, ws_bytes=2048) == _lib.YSMR_ERR_ARG and b"workspace" in L.ysmr_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all()


# ---- through DeviceFrameFeed ---------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name", ["lzw_stack_3x40x52", "lzw_rgb_pred2_40x52", "lzw_white_is_zero_40x52", "packbits_noise_40x52",
                                  "raw_rgb_40x52", "lzw_big_endian_40x52_rows7", "lzw_zeros_300"])
def test_the_feed_delivers_the_recorded_frames_without_pillow(tmp_path, monkeypatch, name):
    from ysmr_amd.frames import TiffVideo
    monkeypatch.setitem(sys.modules, "PIL", None)                            # Pillow cannot be imported

    def no_host(self, k, dst):
        raise AssertionError("the host decoded a page")

    monkeypatch.setattr(TiffVideo, "_decode_page", no_host)
    _, data, frames = entry(name)
    video = opened(tmp_path, data)
    assert video._Image is None and video.tiff_layout_for(2) is not None
    got = _feed_frames(video, 2)                                             # (the stack: batches of 2 and 1)
    video.close()
    np.testing.assert_array_equal(got, frames)


def _host_path(video, k):
    """What the host path makes of frame k: ('frame', pixels) or ('raises', type, text)."""
    try:
        return ("frame", video.read(k, 1)[0])
    except (OSError, ValueError, SyntaxError) as exc:
        return ("raises", type(exc), str(exc))


def _flagged_file(tmp_path, kind):
    """Five 5 x 2 pages, the fourth one damaged in a way the device flags."""
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (5, 2, 5), dtype=np.uint8)
    if kind == "packbits_run_past_the_end":
        good = [bytes([9]) + f.tobytes() for f in frames]
        bad, compression = bytes([0xFA, 3, 0xFA, 4]), 32773
    elif kind == "lzw_eoi_before_full":
        good = [tm.lzw_literals(f.tobytes()) for f in frames]
        bad, compression = tm.lzw_literals(frames[3].tobytes()[:6]), 5
    else:
        good = [f.tobytes() for f in frames]
        bad, compression = frames[3].tobytes()[:7], 1
    pages = [tt.page(5, 2, [bad if k == 3 else good[k]], compression=compression) for k in range(5)]
    return tt.write_tiff(tmp_path / "f.tif", pages, odd=True), frames


@pytest.mark.parametrize("kind", ["packbits_run_past_the_end", "lzw_eoi_before_full", "raw_short"])
def test_the_feed_sends_flagged_frames_to_the_host_path(tmp_path, kind):
    """A frame the device flags is decoded by the host path: it arrives as that path decodes it, or the feed raises what that
    path raises (Pillow's error; the reader's ValueError where Pillow is absent, and for an uncompressed strip that is short)."""
    from ysmr_amd.frames import TiffVideo
    path, frames = _flagged_file(tmp_path, kind)
    video = TiffVideo(path)
    assert video.tiff_layout_for(4) is not None
    host = _host_path(video, 3)
    try:
        if host[0] == "raises":
            with pytest.raises(host[1]) as caught:
                _feed_frames(video, 4)
            assert str(caught.value) == host[2]
        else:
            got = _feed_frames(video, 4)
            np.testing.assert_array_equal(got[3], host[1])
            np.testing.assert_array_equal(got[[0, 1, 2, 4]], frames[[0, 1, 2, 4]])
    finally:
        video.close()


def test_the_feed_without_device_decode_is_the_host_path(tmp_path):
    """'hip decode tiff' False: the same frames, by the host path (an uncompressed file needs no Pillow there; an LZW file gives
    what that path gives)."""
    from ysmr_amd.frames import decode_tiff_setting
    off = decode_tiff_setting({"hip decode tiff": False})
    assert off is False
    for name in ("raw_noise_40x52", "lzw_stack_3x40x52"):
        _, data, frames = entry(name)
        video = opened(tmp_path, data, name + ".tif")
        host = _host_path(video, 0)
        try:
            if host[0] == "raises":
                assert name.startswith("lzw")
                with pytest.raises(host[1]):
                    _feed_frames(video, 2, decode_tiff=off)
            else:
                np.testing.assert_array_equal(_feed_frames(video, 2, decode_tiff=off), frames)
            np.testing.assert_array_equal(_feed_frames(video, 2, decode_tiff=True), frames)
        finally:
            video.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip():
    """(frames u8 [64, 96, 128] of a small synthetic clip, the bytes of its LZW TIFF: strips of 16 rows from the model's encoder)."""
    from ysmr_amd.synth import SyntheticVideo
    frames = SyntheticVideo(96, 128, 8, seed=4).frames(64)
    pages = [tt.page(128, 96, [tm.lzw_encode(f[r:r + 16].tobytes()) for r in range(0, 96, 16)], rows_per_strip=16, compression=5)
             for f in frames]
    frames.setflags(write=False)
    return frames, tt.tiff_bytes(pages)


def _settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False,
                            "log to file": False, "minimal frame count": 40})
    s.update(kw)
    return s


def test_track_bacteria_from_an_lzw_tiff(tmp_path):
    """The same ``_list.csv`` bytes from the LZW TIFF, on the device path and on the host path's setting, as from the .npy."""
    from ysmr_amd.track_eval import track_bacteria
    frames, data = _clip()
    for sub in ("t", "n"):
        os.makedirs(tmp_path / sub)
    (tmp_path / "t" / "clip.tif").write_bytes(data)
    np.save(tmp_path / "n" / "clip.npy", frames)
    rt = track_bacteria(str(tmp_path / "t" / "clip.tif"), settings=_settings(**{"hip decode tiff": True}), result_folder=str(tmp_path / "t"),
                        batch=16)
    rn = track_bacteria(str(tmp_path / "n" / "clip.npy"), settings=_settings(), result_folder=str(tmp_path / "n"), batch=16)
    assert rt is not None and rn is not None and rt[1:4] == rn[1:4] and rt[2:4] == (96, 128)
    assert len(rt[0]) > 100 and rt[0].equals(rn[0])
    assert open(rt[4], "rb").read() == open(rn[4], "rb").read()


def test_annotate_video_reads_a_tiff(tmp_path):
    import pandas as pd
    from ysmr_amd import annotate_video
    frames, _ = _clip()
    rows = [(7, t, 20.0 + t, 30.0 + 0.5 * t, 1, 0, 2) for t in range(12)] + [(9, t, 90.0 - t, 60.0, 0, 0, 0) for t in range(3, 12)]
    df = pd.DataFrame(rows, columns=["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "moving", "turn_points", "motility_phenotype"])
    df = df.astype({"TRACK_ID": np.int64, "POSITION_T": np.int64, "moving": np.int8, "turn_points": np.int8, "motility_phenotype": np.int8})
    written = {}
    for sub in ("t", "n"):
        os.makedirs(tmp_path / sub)
        if sub == "t":
            pages = [tt.page(128, 96, [tm.lzw_encode(f.tobytes())], compression=5) for f in frames[:12]]
            path = tt.write_tiff(tmp_path / sub / "clip.tif", pages, byteorder=">", odd=True)
        else:
            path = str(tmp_path / sub / "clip.npy")
            np.save(path, frames[:12])
        s = _settings(**{"hip frames per batch": 5, "frames per second": 25.0})
        written[sub] = annotate_video(path, df, settings=s, result_folder=str(tmp_path / sub / "out"))
        assert written[sub] is not None and os.path.isfile(written[sub])
    assert open(written["t"], "rb").read() == open(written["n"], "rb").read()
