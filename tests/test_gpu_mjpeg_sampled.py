"""``ysmr_mjpeg_encode_batch`` -- 4:4:4 / 4:2:2 / 4:2:0, the Annex K.3 tables or tables built per frame -- and
``annotate_video`` with the two settings keys, on the device against the model of tests/jpeg_sampled_model.py: every byte of
every chunk must be equal."""
import functools
import io
import logging
import os

import numpy as np
import pytest

import annotate_model as am
import jpeg_sampled_model as jsm
from test_gpu_mjpeg import _assert_chunks, _payloads, frames_of

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (8, 8), (9, 17), (16, 40), (23, 41), (37, 50), (24, 539))
MODES = tuple((s, h) for s in (1, 2, 3) for h in (0, 1))
#: 1 and 90 everywhere, 50 and 100 on two shapes
CASES = tuple((shape, q) for shape in SHAPES for q in ((1, 50, 90, 100) if shape in ((9, 17), (23, 41)) else (1, 90)))


@functools.lru_cache(maxsize=None)
def five_frames(shape):
    """Five frames of different content: those of test_gpu_mjpeg.frames_of (flat, noise, saturated, checkerboard, and the
    painted frame where there is one), a second noise frame where there is none."""
    frames = frames_of(shape)
    if len(frames) < 5:
        extra = np.random.default_rng(shape[0] * 7 + shape[1]).integers(0, 256, (1,) + shape + (3,), dtype=np.uint8)
        frames = np.concatenate([frames, extra])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def chunks_of(shape, quality, sampling, huffman):
    return tuple(jsm.chunk(jsm.encode(f, quality, sampling, huffman)) for f in five_frames(shape))


def launch(frames, quality, bottom_up, sampling, huffman, stride=None, gap=0, capacity=None, guard=64):
    """One ``ysmr_mjpeg_encode_batch``: (out bytes with the guard, offsets [n + 1], status)."""
    import torch
    from ysmr_amd import _lib
    n, h, w = frames.shape[:3]
    stride = (3 * w + 3) & ~3 if stride is None else stride
    frame_bytes = stride * h + gap
    dib = am.pack_dib(frames, bottom_up, stride=stride, frame_bytes=frame_bytes, fill=0x5C)
    dev = torch.device("cuda:0")
    L = _lib.lib()
    ws_bytes = L.ysmr_mjpeg_encode_workspace_bytes(n, h, w, sampling, huffman)
    assert ws_bytes > 0
    dib_dev = torch.from_numpy(np.ascontiguousarray(dib)).to(dev)
    ws = torch.full((ws_bytes,), 0xEE, dtype=torch.uint8, device=dev)          # (the kernels may rely on nothing in it)
    capacity = n * stride * h if capacity is None else capacity
    out = torch.full((capacity + guard,), 0xAA, dtype=torch.uint8, device=dev)
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = L.ysmr_mjpeg_encode_batch(_lib.stream_ptr(dev), dib_dev.data_ptr(), n, h, w, stride, frame_bytes, int(bottom_up), quality,
                                   sampling, huffman, ws.data_ptr(), ws_bytes, out.data_ptr(), capacity, offsets.data_ptr(),
                                   status.data_ptr())
    _lib.check(rc, "ysmr_mjpeg_encode_batch")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), offsets.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("bottom_up", [1, 0])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: "s{}h{}".format(*m))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}x{}-q{}".format(c[0][0], c[0][1], c[1]))
def test_chunks_equal_the_model_byte_for_byte(case, mode, bottom_up):
    (shape, quality), (sampling, huffman) = case, mode
    frames, want = five_frames(shape), chunks_of(shape, quality, sampling, huffman)
    capacity = sum(len(c) for c in want) + 100
    out, offsets, status = launch(frames, quality, bottom_up, sampling, huffman, capacity=capacity)
    assert status == 0
    _assert_chunks(out, offsets, want, "{} q{} sampling {} huffman {} bottom_up={}".format(shape, quality, sampling, huffman, bottom_up))
    assert (out[offsets[-1]:] == 0xAA).all()                                   # nothing behind the last chunk


@pytest.mark.parametrize("sampling", [1, 3])
def test_the_noise_frame_eight_times_gives_eight_identical_chunks(sampling):
    shape = (37, 50)
    eight = np.repeat(five_frames(shape)[1:2], 8, axis=0)
    want = chunks_of(shape, 90, sampling, 1)[1]
    first = launch(eight, 90, 1, sampling, 1)
    assert first[2] == 0
    _assert_chunks(first[0], first[1], (want,) * 8, "eight noise frames")
    again = launch(eight, 90, 1, sampling, 1)
    assert again[2] == 0 and np.array_equal(first[1], again[1]) and np.array_equal(first[0], again[0])


def test_capacity_contract():
    shape = (23, 41)
    noise = np.stack([np.random.default_rng(k).integers(0, 256, shape + (3,), dtype=np.uint8) for k in range(4)])
    want = tuple(jsm.chunk(jsm.encode(f, 100, 3, 1)) for f in noise)
    total = sum(len(c) for c in want)
    cut_at = (int(np.cumsum([len(c) for c in want])[1]) + total) // 2 & ~3      # two chunks fit, the last does not
    cut_at = min(cut_at, total - 5)
    out, offsets, status = launch(noise, 100, 1, 3, 1, capacity=cut_at)
    assert status & 1
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want])]).tolist()
    assert (out[cut_at:] == 0xAA).all() and len(out) == cut_at + 64
    inside = [i for i in range(4) if offsets[i + 1] <= cut_at]
    assert inside and len(inside) < 4
    for i in inside:
        assert out[offsets[i]:offsets[i + 1]].tobytes() == want[i]
    cut = len(inside)                                                          # the chunk the capacity cuts: right as far as it goes
    assert out[offsets[cut]:cut_at].tobytes() == want[cut][:cut_at - offsets[cut]]
    out, offsets, status = launch(noise, 100, 1, 3, 1, capacity=total)
    assert status == 0
    _assert_chunks(out, offsets, want, "exact capacity")
    assert (out[total:] == 0xAA).all()


@pytest.mark.parametrize("mode", [(2, 1), (3, 0)], ids=lambda m: "s{}h{}".format(*m))
def test_a_stride_and_a_gap_of_the_callers_choosing(mode):
    shape = (23, 41)
    frames, want = five_frames(shape), chunks_of(shape, 90, *mode)
    stride = ((3 * 41 + 3) & ~3) + 8
    out, offsets, status = launch(frames, 90, 0, *mode, stride=stride, gap=12, capacity=sum(len(c) for c in want))
    assert status == 0
    _assert_chunks(out, offsets, want, "stride + 8, gap 12")


def test_bad_arguments_are_refused():
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    ws_bytes = L.ysmr_mjpeg_encode_workspace_bytes(1, 16, 24, 3, 1)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    meta = torch.zeros(4, dtype=torch.int64, device=dev)
    good = dict(dib=buf.data_ptr(), n=1, h=16, w=24, stride=72, frame_bytes=72 * 16, quality=90, sampling=3, huffman=1, ws=ws.data_ptr(),
                ws_bytes=ws_bytes, out=buf.data_ptr() + 4096, cap=8192, offsets=meta.data_ptr(), status=meta.data_ptr() + 16)

    def call(**change):
        a = dict(good, **change)
        return L.ysmr_mjpeg_encode_batch(_lib.stream_ptr(dev), a["dib"], a["n"], a["h"], a["w"], a["stride"], a["frame_bytes"], 1,
                                         a["quality"], a["sampling"], a["huffman"], a["ws"], a["ws_bytes"], a["out"], a["cap"],
                                         a["offsets"], a["status"])

    for change in (dict(sampling=0), dict(sampling=4), dict(huffman=2), dict(huffman=-1), dict(ws_bytes=ws_bytes - 1), dict(dib=None),
                   dict(ws=None), dict(out=None), dict(offsets=None), dict(status=None), dict(quality=0), dict(n=0)):
        assert call(**change) == _lib.YSMR_ERR_ARG, change
    for sampling, huffman in ((0, 0), (4, 0), (1, 2), (1, -1)):
        assert L.ysmr_mjpeg_encode_workspace_bytes(1, 16, 24, sampling, huffman) == 0
    assert call() == _lib.YSMR_OK
    torch.cuda.synchronize(dev)
    want = jsm.chunk(jsm.encode(np.zeros((16, 24, 3), np.uint8), 90, 3, 1))
    assert int(meta[2].item()) == 0 and int(meta[1].item()) == len(want)


def test_workspace_sizes():
    from ysmr_amd import _lib
    L = _lib.lib()
    for n, h, w in ((1, 16, 24), (5, 48, 64), (8, 1080, 1920), (3, 37, 50)):
        today = L.ysmr_mjpeg_workspace_bytes(n, h, w)
        assert 0 < L.ysmr_mjpeg_encode_workspace_bytes(n, h, w, 1, 0) <= today
    for n, h, w in ((5, 48, 64), (8, 1080, 1920)):                             # several MCUs
        today = L.ysmr_mjpeg_workspace_bytes(n, h, w)
        assert L.ysmr_mjpeg_encode_workspace_bytes(n, h, w, 3, 0) < today
        assert L.ysmr_mjpeg_encode_workspace_bytes(n, h, w, 2, 0) < today
    big = (8, 1080, 1920)
    assert L.ysmr_mjpeg_encode_workspace_bytes(*big, 3, 0) <= 0.51 * L.ysmr_mjpeg_workspace_bytes(*big)   # 1.5 blocks of 3


def _pillow(jpeg):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))[..., ::-1]


@pytest.mark.parametrize("sampling", [3, 2])
def test_round_trip_through_the_device_decoder(sampling):
    pytest.importorskip("PIL")
    import torch
    from ysmr_amd import _lib
    shape = (23, 41)
    frames = five_frames(shape)
    n, (h, w) = len(frames), shape
    out, offsets, status = launch(frames, 90, 1, sampling, 1)
    assert status == 0
    dev = torch.device("cuda:0")
    L = _lib.lib()
    # the decoder takes the chunks' bodies back to back: the JPEGs without '00dc' and the size
    jpegs = [out[offsets[i] + 8:offsets[i] + 8 + int.from_bytes(out[offsets[i] + 4:offsets[i] + 8].tobytes(), "little")] for i in range(n)]
    chunks_dev = torch.from_numpy(np.concatenate(jpegs)).to(dev)
    offsets_dev = torch.from_numpy(np.concatenate([[0], np.cumsum([len(j) for j in jpegs])]).astype(np.int64)).to(dev)
    ws_bytes = L.ysmr_mjpeg_decode_workspace_bytes(n, h, w, 3, sampling)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xEE, dtype=torch.uint8, device=dev)
    pixels = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=dev)
    flags = torch.full((n,), -1, dtype=torch.int32, device=dev)
    _lib.check(L.ysmr_mjpeg_decode_batch(_lib.stream_ptr(dev), chunks_dev.data_ptr(), offsets_dev.data_ptr(), n, h, w, 3, sampling,
                                         ws.data_ptr(), ws_bytes, pixels.data_ptr(), flags.data_ptr()), "ysmr_mjpeg_decode_batch")
    torch.cuda.synchronize(dev)
    assert flags.cpu().tolist() == [0] * n
    got = pixels.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], _pillow(jpegs[i].tobytes())), "frame {}".format(i)


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_annotate_video_writes_420_with_built_tables(tmp_path, caplog):
    from test_gpu_annotate import _clip_and_table, _expected
    from ysmr_amd import annotate_video
    from ysmr_amd.helper_file import default_settings
    clip, df, per_frame = _clip_and_table()
    path = str(tmp_path / "clip.npy")
    np.save(path, clip)
    out = str(tmp_path / "results")
    s = default_settings(**{"log to file": False, "hip frames per batch": 5, "frames per second": 25.0, "log_level": logging.INFO,
                            "save video file extension": ".avi", "save video fourcc codec": "MJPG",
                            "hip video jpeg subsampling": "4:2:0", "hip video jpeg huffman": "optimised"})
    with caplog.at_level(logging.INFO, logger="ysmr"):
        written = annotate_video(path, df, settings=s, result_folder=out)      # three batches: 5, 5 and 2 frames
    assert written == os.path.join(out, "clip_annotated_output.avi") and os.path.isfile(written)
    assert "Motion-JPEG, quality 90, 4:2:0, optimised Huffman tables" in caplog.text
    model = [jsm.encode(f, 90, 3, 1) for f in _expected(clip, per_frame)]
    got = _payloads(written)
    assert len(got) == 12
    for i in range(12):
        assert got[i] == model[i], "frame {}".format(i)

    pytest.importorskip("PIL")
    from ysmr_amd.frames import AviVideo
    video = AviVideo(written)
    assert (video.frame_count, video.frames_available, video.height, video.width) == (12, 12, 48, 64)
    frames = video.read(0, 12)
    video.close()
    for i in range(12):
        assert np.array_equal(np.asarray(frames[i]).reshape(48, 64, 3), _pillow(model[i])), "frame {}".format(i)


def test_a_batch_larger_than_its_raw_size_is_encoded_again(tmp_path, caplog):
    import pandas as pd
    from avi_tools import write_avi
    from ysmr_amd import annotate_video
    from ysmr_amd.helper_file import default_settings
    # (noise at 4:2:2 with tables of its own takes about 20 bits per pixel, fewer than the raw frame's 24: it is the header
    # that makes a frame this small larger than its raw size)
    clip = np.random.default_rng(3).integers(0, 256, (7, 8, 24, 3), dtype=np.uint8)
    model = [jsm.encode(f, 100, 2, 1) for f in clip]
    assert sum(len(jsm.chunk(j)) for j in model[:5]) > 5 * 8 * 72              # the first batch does not fit its default buffer
    path = str(tmp_path / "noise.avi")
    write_avi(path, clip, bits=24, fps=(25, 1))
    df = pd.DataFrame({"TRACK_ID": np.array([], np.int64), "POSITION_T": np.array([], np.int64), "POSITION_X": np.array([], np.float64),
                       "POSITION_Y": np.array([], np.float64), "moving": np.array([], np.int8), "turn_points": np.array([], np.int8),
                       "motility_phenotype": np.array([], np.int8)})
    s = default_settings(**{"log to file": False, "hip frames per batch": 5, "frames per second": 25.0, "hip video jpeg quality": 100,
                            "hip video jpeg subsampling": "4:2:2", "hip video jpeg huffman": "optimised",
                            "save video file extension": ".avi", "save video fourcc codec": "mjpg", "log_level": logging.DEBUG})
    with caplog.at_level(logging.DEBUG, logger="ysmr"):
        written = annotate_video(path, df, settings=s, result_folder=str(tmp_path / "results"))
    assert written is not None and "encoding them again" in caplog.text
    assert "4:2:2, optimised Huffman tables" in caplog.text
    assert _payloads(written) == model


@pytest.mark.parametrize("key, value", [("hip video jpeg subsampling", "4:1:1"), ("hip video jpeg subsampling", 420),
                                        ("hip video jpeg huffman", "optimal"), ("hip video jpeg huffman", True)])
def test_a_bad_value_of_a_settings_key_is_a_value_error_before_any_file(tmp_path, key, value, caplog):
    from test_gpu_annotate import _clip_and_table
    from ysmr_amd import annotate_video
    from ysmr_amd.annotate import output_format
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"log to file": False, "save video file extension": ".avi", "save video fourcc codec": "MJPG", key: value})
    with pytest.raises(ValueError) as err:
        output_format(s)
    assert key in str(err.value) and repr(value) in str(err.value)
    clip, df, _ = _clip_and_table()
    path = str(tmp_path / "clip.npy")
    np.save(path, clip)
    out = str(tmp_path / "results")
    with caplog.at_level(logging.CRITICAL, logger="ysmr"):
        assert annotate_video(path, df, settings=s, result_folder=out) is None     # (as for the quality: logged, nothing written)
    assert key in caplog.text and (not os.path.isdir(out) or os.listdir(out) == [])
