"""The Motion-JPEG decoder's NumPy model (tests/jpeg_decode_model.py) against Pillow -- recorded in the fixture
tests/golden/mjpeg_decode_streams.npz, and live where Pillow can be imported --, the status it gives unsupported and damaged
streams, and the host side of the device path: ``AviVideo.jpeg_layout`` / ``read_jpeg_into``.  No GPU."""
import functools
import io
import json
import os

import numpy as np
import pytest

import jpeg_decode_model as dm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mjpeg_decode_streams.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    """[(entry of the index, stream bytes, Pillow's pixels or None)], read once and shared."""
    with np.load(FIXTURE) as z:
        index = json.loads(bytes(z["index"]).decode())
        out = []
        for e in index:
            pixels = z["pixels_" + e["name"]] if e["status"] == 0 else None
            if pixels is not None:
                pixels.setflags(write=False)
            out.append((e, bytes(z["jpeg_" + e["name"]]), pixels))
    return out


@functools.lru_cache(maxsize=None)
def modelled(name):
    """(status, pixels) of the model for a fixture stream, worked out once."""
    e, stream, _ = next(item for item in fixture() if item[0]["name"] == name)
    status, pixels = dm.decode(stream, e["height"], e["width"], e["sampling"])
    pixels.setflags(write=False)
    return status, pixels


def names(supported=None):
    with np.load(FIXTURE) as z:
        index = json.loads(bytes(z["index"]).decode())
    return [e["name"] for e in index if supported is None or (e["status"] == 0) == supported]


def test_the_fixture_holds_what_the_issue_lists():
    entries = [e for e, _, _ in fixture()]
    good = [e for e in entries if e["status"] == 0]
    assert {(e["height"], e["width"]) for e in good} == {(8, 8), (9, 17), (23, 41), (16, 40), (31, 33), (24, 539)}
    for s, label in enumerate(("L", "444", "422", "420")):
        mine = [e["name"] for e in good if e["sampling"] == s]
        assert all(n.startswith(label) for n in mine)
        for option in ("plain", "optimize", "rows", "blocks", "nodht"):
            assert any("_" + option + "_" in n for n in mine), (label, option)
        for quality in (1, 50, 90, 100):
            assert any("_q{}_".format(quality) in n for n in mine), (label, quality)
        for kind in ("flat", "noise", "saturated", "checkerboard"):
            assert any(n.endswith(kind) for n in mine), (label, kind)
    assert sorted(e["name"] for e in entries if e["status"]) == [
        "420_rst_overwritten_23x41", "444_app14_23x41", "444_cut_in_half_23x41", "444_dqt16_23x41", "444_progressive_23x41"]
    assert os.path.getsize(FIXTURE) < 576 * 1024


@pytest.mark.parametrize("name", names(supported=True))
def test_the_model_equals_pillows_recorded_pixels(name):
    e, _, pixels = next(item for item in fixture() if item[0]["name"] == name)
    status, mine = modelled(name)
    assert status == 0
    assert mine.shape == pixels.shape == ((e["height"], e["width"]) if e["sampling"] == 0 else (e["height"], e["width"], 3))
    np.testing.assert_array_equal(mine, pixels)


def test_the_range_limit_stream_leaves_the_sample_range():
    """The hand-built stream is there to tell a clamp from the portable code's wrapping table: many of its samples lie
    beyond +-512 before they are limited, some first-pass results beyond 16 bits."""
    e, stream, _ = next(item for item in fixture() if item[0]["name"] == "420_range_limit_31x33")
    quant, tables, slots, ri, start = dm._headers(stream, e["height"], e["width"], 3)
    coef = dm._coefficients(stream, e["height"], e["width"], 3, tables, slots, ri, start)
    d = (coef[1] * quant[1]).reshape(coef[1].shape[:-1] + (8, 8))
    first = np.swapaxes(dm._pass(np.swapaxes(d, -1, -2), 11), -1, -2)
    assert np.abs(dm._pass(first, 18)).max() > 512
    luma = (coef[0] * quant[0]).reshape(coef[0].shape[:-1] + (8, 8))
    assert np.abs(np.swapaxes(dm._pass(np.swapaxes(luma, -1, -2), 11), -1, -2)).max() > 32767
    assert np.abs(coef[2] * quant[2]).max() > 32767


@pytest.mark.parametrize("name", names(supported=False))
def test_unsupported_and_damaged_streams_get_their_status(name):
    e, _, _ = next(item for item in fixture() if item[0]["name"] == name)
    assert modelled(name)[0] == e["status"]
    assert e["status"] == (dm.UNSUPPORTED if name.split("_")[1] in ("progressive", "app14", "dqt16") else dm.CORRUPT)


def test_more_status_rules():
    e, stream, _ = next(item for item in fixture() if item[0]["name"] == "L_rows_23x41_q50_saturated")     # RST0, RST1
    h, w = e["height"], e["width"]
    assert dm.decode(stream, h, w, 0)[0] == 0
    assert dm.decode(stream, h, w + 1, 0)[0] == dm.UNSUPPORTED           # geometry other than the call's
    assert dm.decode(stream, h, w, 1)[0] == dm.UNSUPPORTED               # sampling other than the call's
    assert dm.decode(stream[2:], h, w, 0)[0] == dm.CORRUPT               # no SOI
    assert dm.decode(b"\xff\xd8\xff\xd9", h, w, 0)[0] == dm.CORRUPT      # no SOS
    at = stream.index(b"\xff\xd1")
    assert dm.decode(stream[:at + 1] + b"\xd3" + stream[at + 2:], h, w, 0)[0] == dm.CORRUPT      # RST out of sequence
    assert dm.decode(stream[:at] + stream[at + 2:], h, w, 0)[0] == dm.CORRUPT                     # RST missing
    assert dm.decode(stream + b"\x00", h, w, 0)[0] == 0                  # a pad byte behind EOI
    assert dm.decode(stream[:2] + b"\xff\xff" + stream[2:], h, w, 0)[0] == 0                     # fill bytes before a marker
    at = stream.index(b"\xff\xdb")
    size = int.from_bytes(stream[at + 2:at + 4], "big")
    assert dm.decode(stream[:at] + stream[at + 2 + size:], h, w, 0)[0] == dm.CORRUPT             # no DQT the scan needs
    sos = stream.index(b"\xff\xda")
    assert dm.decode(stream[:sos + 4] + b"\x02" + stream[sos + 5:], h, w, 0)[0] == dm.CORRUPT     # Ns against the length
    with pytest.raises(ValueError):
        dm.decode(stream, h, w, 4)


@pytest.mark.parametrize("name", names(supported=True))
def test_the_model_equals_a_live_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    e, stream, _ = next(item for item in fixture() if item[0]["name"] == name)
    with Image.open(io.BytesIO(stream)) as im:
        live = np.asarray(im.convert("L")) if e["sampling"] == 0 else np.asarray(im.convert("RGB"))[:, :, ::-1]
    np.testing.assert_array_equal(modelled(name)[1], live)


@pytest.mark.parametrize("quality", (50, 90, 100))
@pytest.mark.parametrize("name", ["scene37x50", "noise23x41", "saturated16x40", "flat8x8"])
def test_the_model_decodes_the_encoders_streams_as_pillow_does(name, quality):
    Image = pytest.importorskip("PIL.Image")
    import test_mjpeg_cpu
    bgr = test_mjpeg_cpu.images()[name]
    stream, _ = test_mjpeg_cpu.encoded(name, quality)
    status, mine = dm.decode(stream, bgr.shape[0], bgr.shape[1], 1)
    assert status == 0
    with Image.open(io.BytesIO(stream)) as im:
        np.testing.assert_array_equal(mine, np.asarray(im.convert("RGB"))[:, :, ::-1])


def test_truncated_streams_are_what_pillow_refuses():
    Image = pytest.importorskip("PIL.Image")
    _, stream, _ = next(item for item in fixture() if item[0]["name"] == "444_cut_in_half_23x41")
    with pytest.raises(OSError, match="truncated"):
        with Image.open(io.BytesIO(stream)) as im:
            im.load()


def test_the_fixture_regenerates_identically(tmp_path):
    pytest.importorskip("PIL.Image")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_mjpeg_streams", os.path.join(os.path.dirname(FIXTURE), "gen_mjpeg_streams.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.write(str(tmp_path / "again.npz"))
    assert open(tmp_path / "again.npz", "rb").read() == open(FIXTURE, "rb").read()


def _avi(tmp_path, names_, h, w):
    from avi_tools import write_avi
    blobs = [next(s for e, s, _ in fixture() if e["name"] == n) for n in names_]
    path = tmp_path / "m.avi"
    write_avi(path, np.zeros((len(blobs), h, w), np.uint8), 24, fps=(25, 1), jpeg=blobs)
    return str(path), blobs


def test_jpeg_layout_and_read_jpeg_into(tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from ysmr_amd.frames import AviVideo
    # (an odd-sized chunk first: the RIFF pad byte behind it is not part of the next frame)
    path, blobs = _avi(tmp_path, ["420_rst_overwritten_23x41", "420_more_23x41_q90_checkerboard", "420_more_23x41_q90_checkerboard",
                                  "420_rst_overwritten_23x41"], 23, 41)
    assert len(blobs[0]) & 1
    v = AviVideo(path)
    try:
        assert (v.frame_count, v.height, v.width, v.channels, v.fps) == (4, 23, 41, 3, 25.0)
        assert v.raw_layout is None
        sizes = [len(b) for b in blobs]
        assert v.jpeg_layout_for(2) == (3, max(sizes), max(sizes[k] + sizes[k + 1] for k in range(3)))
        assert v.jpeg_layout_for(100) == (3, max(sizes), sum(sizes))
        assert v.jpeg_layout == v.jpeg_layout_for(AviVideo.jpeg_batch)
        out, offsets = np.full(sum(sizes) + 5, 0xAA, np.uint8), np.zeros(5, np.int64)
        assert v.read_jpeg_into(0, 4, out, offsets) == 4
        assert list(offsets) == [0] + list(np.cumsum(sizes))
        assert bytes(out[:sum(sizes)]) == b"".join(blobs) and bytes(out[sum(sizes):]) == b"\xaa" * 5
        out[:] = 0xAA
        with ThreadPoolExecutor(3) as pool:
            assert v.read_jpeg_into(1, 7, out, offsets, pool) == 3
        assert list(offsets[:4]) == [0] + list(np.cumsum(sizes[1:]))
        assert bytes(out[:offsets[3]]) == b"".join(blobs[1:])
        # the model decodes what was read, frame by frame
        for k in range(3):
            assert dm.decode(bytes(out[offsets[k]:offsets[k + 1]]), 23, 41, 3)[0] == (dm.CORRUPT if k == 2 else 0)
        with pytest.raises(ValueError):
            v.read_jpeg_into(0, 4, np.zeros(10, np.uint8), offsets)
    finally:
        v.close()


def test_jpeg_layout_is_none_outside_the_subset(tmp_path):
    from avi_tools import write_avi
    from ysmr_amd.frames import AviVideo
    pytest.importorskip("PIL.Image")
    path, _ = _avi(tmp_path, ["444_progressive_23x41"], 23, 41)
    v = AviVideo(path)
    assert v.jpeg_layout is None and v.raw_layout is None and v.channels == 3
    v.close()
    # APP14 and a 16-bit DQT are outside the subset as well: the opening applies the decoder's own header rules
    for name in ("444_app14_23x41", "444_dqt16_23x41"):
        path, _ = _avi(tmp_path, [name] * 3, 23, 41)
        v = AviVideo(path)
        assert v.jpeg_layout is None and v.jpeg_layout_for(3, needs_restart=False) is None and v.channels == 3, name
        v.close()
    # a first frame without a restart interval: supported, but the host path is the faster one
    path, blobs = _avi(tmp_path, ["444_more_23x41_q50_flat", "444_optimize_23x41_q100_saturated"], 23, 41)
    v = AviVideo(path)
    assert v.jpeg_layout is None and v.raw_layout is None and v.channels == 3
    assert v.jpeg_layout_for(248, needs_restart=False) == (1, max(map(len, blobs)), sum(map(len, blobs)))
    v.close()
    write_avi(tmp_path / "raw.avi", np.zeros((2, 8, 8), np.uint8), 8)
    v = AviVideo(str(tmp_path / "raw.avi"))
    assert v.jpeg_layout is None and v.raw_layout is not None
    v.close()


def test_the_opening_agrees_with_the_model_on_every_fixture_stream(tmp_path):
    """``jpeg_layout`` (restart rule aside) is None exactly for the first frames whose HEADERS the model flags; the two damaged
    streams of the fixture have sound headers and are flagged by their entropy data, which the opening does not read."""
    from ysmr_amd.frames import AviVideo
    pytest.importorskip("PIL.Image")
    for e, stream, _ in fixture():
        path, _ = _avi(tmp_path, [e["name"]], e["height"], e["width"])
        v = AviVideo(path)
        layout = v.jpeg_layout_for(1, needs_restart=False)
        v.close()
        try:
            dm._headers(stream, e["height"], e["width"], e["sampling"])
            assert layout == (e["sampling"], len(stream), len(stream)), e["name"]
        except dm._Flag:
            assert layout is None, e["name"]


def test_the_decode_mjpeg_setting():
    from ysmr_amd.frames import decode_mjpeg_setting
    assert decode_mjpeg_setting({}) is True and decode_mjpeg_setting({"hip decode mjpeg": False}) is False
    assert decode_mjpeg_setting({"hip decode mjpeg": "always"}) == "always" and decode_mjpeg_setting({"hip decode mjpeg": "False"}) is False
    assert decode_mjpeg_setting({"hip decode mjpeg": "true"}) is True and decode_mjpeg_setting({"hip decode mjpeg": 1}) is True


def test_a_jpeg_avi_opens_without_pillow(tmp_path, monkeypatch):
    """Pillow absent: a file of the supported subset opens (its frames are the device's business), a flagged frame's host
    decode raises the ValueError the reader raised at opening before, and a file outside the subset is refused."""
    import builtins
    from ysmr_amd.frames import AviVideo
    real = builtins.__import__

    def no_pillow(name, *a, **kw):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **kw)

    name = "L_rows_23x41_q50_saturated"                                     # (a restart interval per MCU row)
    path, blobs = _avi(tmp_path, [name], 23, 41)
    e = next(e for e, s, _ in fixture() if e["name"] == name)
    monkeypatch.setattr(builtins, "__import__", no_pillow)
    v = AviVideo(path)
    assert v.jpeg_layout == (e["sampling"], len(blobs[0]), len(blobs[0])) and v.channels == (1 if e["sampling"] == 0 else 3)
    with pytest.raises(ValueError, match="needs Pillow"):
        v.read(0, 1)
    v.close()
    for name in ("444_progressive_23x41", "444_more_23x41_q50_flat"):       # outside the subset; no restart interval
        bad, _ = _avi(tmp_path, [name], 23, 41)
        with pytest.raises(ValueError, match="needs Pillow"):
            AviVideo(bad)
