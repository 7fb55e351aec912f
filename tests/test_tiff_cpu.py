"""CPU: the model of the TIFF strip decoders (tests/tiff_decode_model.py) against Pillow and against the recorded files of
tests/golden/tiff_decode_streams.npz; ``frames.TiffVideo`` -- the directories it parses, what it refuses and with which words,
its host path against Pillow --; ``open_video`` for ``.tif``; the settings key 'hip decode tiff'.  Nothing runs on a GPU."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import tiff_decode_model as tm
import tiff_tools as tt

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def fixture():
    """[(name, file bytes, frames u8 [T, H, W(, 3)])] of tests/golden/tiff_decode_streams.npz, frames read-only."""
    out = []
    with np.load(os.path.join(HERE, "golden", "tiff_decode_streams.npz")) as z:
        for name in json.loads(bytes(z["index"]).decode()):
            frames = z["frames_" + name]
            frames.setflags(write=False)
            out.append((name, bytes(z["file_" + name]), frames))
    return out


def names():
    return [name for name, _, _ in fixture()]


def entry(name):
    return next(e for e in fixture() if e[0] == name)


def opened(tmp_path, data, name="clip.tif"):
    from ysmr_amd.frames import TiffVideo
    path = tmp_path / name
    path.write_bytes(data)
    return TiffVideo(str(path))


def bodies_of(video, data, k):
    offsets, counts = video.strips_of(k)
    return [data[int(o):int(o) + int(c)] for o, c in zip(offsets, counts)]


def modelled(video, data, k):
    return tm.decode_frame(bodies_of(video, data, k), video._rows_per_strip, video.height, video.width, video.channels,
                           video._compression, video._predictor, video._photometric)


# ---- hand-built streams: (name, width, height, compression, strip body, status the model gives) ----------------------------------
def hand_built():
    C, E = (tm.CLEAR, 9), (tm.EOI, 9)
    lit = [(v, 9) for v in (10, 20, 30, 40, 50, 60, 70, 80)]
    out = [
        ("lzw_no_leading_clear", 4, 2, 5, tm.pack_codes(lit + [E]), 0),
        ("lzw_eoi_before_full", 4, 2, 5, tm.pack_codes([C] + lit[:5] + [E]), tm.SHORT),
        ("lzw_no_eoi_but_full", 4, 2, 5, tm.pack_codes([C] + lit), 0),
        # 10, 20, 258 (= 10 20), 259 (= 20 10), then 261, the next free entry: (20 10) + 20, of which two bytes still fit
        ("lzw_strings", 4, 2, 5, tm.pack_codes([C, (10, 9), (20, 9), (258, 9), (259, 9), (261, 9), E]), 0),
        ("lzw_kwkwk", 4, 2, 5, tm.pack_codes([C, (7, 9), (258, 9), (259, 9), (7, 9), (7, 9), E]), 0),
        ("lzw_code_above_free", 4, 2, 5, tm.pack_codes([C, (10, 9), (20, 9), (260, 9), (30, 9), E]), tm.BAD_CODE),
        ("lzw_first_code_not_clear", 4, 2, 5, tm.pack_codes([(300, 9)] + lit + [E]), tm.BAD_CODE),
        ("lzw_string_after_clear", 4, 2, 5, tm.pack_codes([C, (10, 9), C, (258, 9), E]), tm.BAD_CODE),
        ("lzw_cut_mid_code", 4, 2, 5, tm.pack_codes([C] + lit[:6])[:-1], tm.SHORT),
        ("lzw_string_past_the_end", 3, 1, 5, tm.pack_codes([C, (1, 9), (2, 9), (258, 9)]), 0),
        ("lzw_old_style", 4, 2, 5, bytes([0, 1, 10, 20, 30]), tm.OLD_LZW),
        ("lzw_empty", 4, 2, 5, b"", tm.SHORT),
        ("packbits_mixed", 5, 2, 32773, bytes([2, 1, 2, 3, 0x80, 0xFD, 9, 0, 4, 0xFF, 5]), 0),       # 1 2 3 / no-op / 9 x 4 / 4 / 5 5
        ("packbits_run_past_the_end", 5, 2, 32773, bytes([0xFA, 3, 0xFA, 4]), tm.OVERRUN),          # 7 + 7 > 10
        ("packbits_literal_past_the_end", 5, 2, 32773, bytes([0xF8, 3, 1, 8, 9]), tm.OVERRUN),      # 9 + 2 > 10
        ("packbits_data_ends", 5, 2, 32773, bytes([0xFC, 3, 4, 1, 2]), tm.SHORT),                   # a literal of 5 with 2 bytes left
        ("packbits_run_without_value", 5, 2, 32773, bytes([0xFC, 3, 0xFC]), tm.SHORT),
        ("raw_short", 5, 2, 1, bytes(range(9)), tm.SHORT),
        ("raw_long", 5, 2, 1, bytes(range(12)), 0),
    ]
    return out


def test_the_hand_built_streams_in_the_model():
    for name, w, h, compression, body, want in hand_built():
        status, data = tm.decode_strip(body, w * h, compression)
        assert status == want, name
        assert len(data) <= w * h, name
    assert tm.decode_strip(hand_built()[0][4], 8, 5)[1] == bytes((10, 20, 30, 40, 50, 60, 70, 80))
    assert tm.lzw_decode(dict((n, b) for n, _, _, _, b, _ in hand_built())["lzw_kwkwk"], 8)[1] == bytes([7] * 8)
    assert tm.lzw_decode(dict((n, b) for n, _, _, _, b, _ in hand_built())["lzw_string_past_the_end"], 3)[1] == bytes([1, 2, 1])
    assert tm.packbits_decode(dict((n, b) for n, _, _, _, b, _ in hand_built())["packbits_mixed"], 10)[1] == bytes([1, 2, 3, 9, 9, 9, 9, 4, 5, 5])


# ---- the model against the recorded files and against Pillow ---------------------------------------------------------------------
@pytest.mark.parametrize("name", names())
def test_the_model_equals_the_recorded_frames(tmp_path, name):
    _, data, frames = entry(name)
    video = opened(tmp_path, data)
    assert video.native and video.frame_count == len(frames)
    for k in range(len(frames)):
        status, frame = modelled(video, data, k)
        assert status == 0
        np.testing.assert_array_equal(frame, frames[k])
    video.close()


def test_the_recorded_lzw_streams_reach_every_branch(tmp_path):
    """The smallest shapes at which the decoder can still go wrong: 12-bit codes and table-full Clears, the KwKwK code alone and
    in bulk with strings longer than a wave, strips at odd offsets with a short last one."""
    seen = {}
    for name in ("lzw_uniform_96", "lzw_gauss_96", "lzw_zeros_300"):
        _, data, frames = entry(name)
        video = opened(tmp_path, data)
        assert video._strips_per_frame == 1
        stats = {}
        assert tm.lzw_decode(bodies_of(video, data, 0)[0], frames[0].size, stats)[0] == 0
        seen[name] = stats
        video.close()
    assert seen["lzw_uniform_96"]["widest"] == 12 and seen["lzw_uniform_96"]["clears"] == 3
    assert seen["lzw_gauss_96"]["widest"] == 12 and seen["lzw_gauss_96"]["clears"] == 2 and seen["lzw_gauss_96"]["kwkwk"] >= 1
    assert seen["lzw_zeros_300"] == dict(codes=425, clears=1, kwkwk=422, widest=10, longest=423)
    _, data, _ = entry("lzw_noise_40x52_rows7")
    video = opened(tmp_path, data)
    offsets, _ = video.strips_of(0)
    assert video._strips_per_frame == 6 and video._rows_per_strip == 7 and any(int(o) & 1 for o in offsets)
    video.close()


def test_the_model_equals_pillow_on_live_files(tmp_path):
    pytest.importorskip("PIL.Image")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gen_tiff_streams as gen
    rng = np.random.default_rng(77)
    made = {
        "lzw": (rng.integers(0, 256, (1, 61, 83), dtype=np.uint8), dict(compression="tiff_lzw"), 5 * 83),
        "lzw_pred": ((rng.integers(0, 5, (2, 61, 83, 3)).cumsum(axis=2) % 256).astype(np.uint8), dict(compression="tiff_lzw", tiffinfo={317: 2}), None),
        "packbits": ((rng.integers(0, 2, (1, 61, 83)) * 200).astype(np.uint8), dict(compression="packbits"), 9 * 83),
        "raw": (rng.integers(0, 256, (2, 61, 83), dtype=np.uint8), dict(compression="raw"), None),
    }
    for name, (frames, kw, strip_bytes) in made.items():
        data = gen.pillow_file(frames, kw, strip_bytes)
        want = gen.pillow_frames(data)
        video = opened(tmp_path, data, name + ".tif")
        assert video.native, name
        for k in range(len(frames)):
            status, frame = modelled(video, data, k)
            assert status == 0, name
            np.testing.assert_array_equal(frame, want[k], err_msg=name)
        np.testing.assert_array_equal(video.read(0, len(frames)), want, err_msg=name)      # the host path
        video.close()


# ---- the parser -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byteorder", ["<", ">"])
@pytest.mark.parametrize("odd", [False, True])
def test_geometry_and_strip_tables(tmp_path, byteorder, odd):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (3, 10, 7), dtype=np.uint8)
    pages = [tt.page(7, 10, [f[0:4].tobytes(), f[4:8].tobytes(), f[8:10].tobytes()], rows_per_strip=4) for f in frames]
    data = tt.tiff_bytes(pages, byteorder=byteorder, odd=odd)
    video = opened(tmp_path, data)
    assert (video.height, video.width, video.channels, video.frame_count, video.frames_available) == (10, 7, 1, 3, 3)
    assert video.native and video._rows_per_strip == 4 and video._strips_per_frame == 3 and video.fps == 30.0
    for k in range(3):
        offsets, counts = video.strips_of(k)
        assert list(counts) == [28, 28, 14]
        assert all(bool(int(o) & 1) == odd for o in offsets)
        for s, (o, c) in enumerate(zip(offsets, counts)):
            assert data[int(o):int(o) + int(c)] == frames[k, 4 * s:4 * s + 4].tobytes()
    np.testing.assert_array_equal(video.read(1, 5), frames[1:])              # uncompressed strips: read without Pillow
    video.close()


def test_a_page_without_rows_per_strip_is_one_strip_and_fps_comes_from_the_caller(tmp_path, caplog):
    import logging
    from ysmr_amd.frames import TiffVideo
    rgb = np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3)
    path = tt.write_tiff(tmp_path / "c.tif", [tt.page(6, 5, [rgb.tobytes()], photometric=2, samples=3)])
    with caplog.at_level(logging.INFO, logger="ysmr"):
        video = TiffVideo(path, default_fps=12.5)
    assert video.fps == 12.5 and any("frame rate" in r.getMessage() for r in caplog.records)
    assert video.channels == 3 and video._strips_per_frame == 1 and video._rows_per_strip == 5
    np.testing.assert_array_equal(video.read(0, 1)[0], rgb[:, :, ::-1])      # B, G, R
    video.close()


def _refused(tmp_path, monkeypatch, pages, **kw):
    """The ValueError text of opening such a file where Pillow cannot be imported."""
    from ysmr_amd.frames import TiffVideo
    monkeypatch.setitem(sys.modules, "PIL", None)
    path = tt.write_tiff(tmp_path / "r.tif", pages, **kw)
    with pytest.raises(ValueError) as caught:
        TiffVideo(path)
    return str(caught.value)


@pytest.mark.parametrize("what, page_kw, words", [
    ("deflate", dict(compression=8), "Compression (259) = 8"),
    ("old deflate", dict(compression=32946), "Compression (259) = 32946"),
    ("jpeg", dict(compression=7), "Compression (259) = 7"),
    ("16 bit", dict(bits=16), "BitsPerSample (258) = 16"),
    ("palette", dict(photometric=3), "PhotometricInterpretation (262) = 3"),
    ("tiles", dict(extra={322: (tt.SHORT, [16])}), "TileWidth (322) = 16"),
    ("planar", dict(photometric=2, samples=3, extra={284: (tt.SHORT, [2])}), "PlanarConfiguration (284) = 2"),
    ("extra samples", dict(photometric=2, samples=3, extra={338: (tt.SHORT, [1])}), "ExtraSamples (338)"),
    ("two samples", dict(samples=2), "SamplesPerPixel (277) = 2"),
    ("predictor 3", dict(predictor=3), "Predictor (317) = 3"),
    ("lsb fill order", dict(extra={266: (tt.SHORT, [2])}), "FillOrder (266) = 2"),
])
def test_what_is_outside_the_subset_names_its_tag_without_pillow(tmp_path, monkeypatch, what, page_kw, words):
    samples = page_kw.get("samples", 1)
    text = _refused(tmp_path, monkeypatch, [tt.page(4, 2, [bytes(8 * samples)], **page_kw)])
    assert words in text and "Pillow" in text, text


def test_old_style_lzw_and_a_page_unlike_the_first(tmp_path, monkeypatch):
    text = _refused(tmp_path, monkeypatch, [tt.page(4, 2, [bytes([0, 1, 2, 3])], compression=5)])
    assert "Compression (259) = 5 in its old LSB-first form" in text
    # a later page of another size: the file opens, the page is Pillow's -- and without Pillow an error naming the tag
    from ysmr_amd.frames import TiffVideo
    monkeypatch.setitem(sys.modules, "PIL", None)
    path = tt.write_tiff(tmp_path / "d.tif", [tt.page(4, 2, [bytes(range(8))]), tt.page(4, 3, [bytes(12)])])
    video = TiffVideo(path)
    assert not video.native and video.tiff_layout_for(2) is None
    np.testing.assert_array_equal(video.read(0, 1)[0], np.arange(8, dtype=np.uint8).reshape(2, 4))
    with pytest.raises(ValueError) as caught:
        video.read(1, 1)
    assert "ImageLength (257) = 3, the first page has 2" in str(caught.value) and "Pillow" in str(caught.value)
    video.close()


def test_bigtiff_and_other_files_are_refused_at_opening(tmp_path):
    from ysmr_amd.frames import TiffVideo
    path = tt.write_tiff(tmp_path / "b.tif", [tt.page(4, 2, [bytes(8)])], version=43)
    with pytest.raises(ValueError, match="BigTIFF"):
        TiffVideo(path)
    (tmp_path / "n.tif").write_bytes(b"RIFF1234AVI LIST")
    with pytest.raises(ValueError, match="not a TIFF file"):
        TiffVideo(str(tmp_path / "n.tif"))
    data = tt.tiff_bytes([tt.page(4, 2, [bytes(8)])])
    (tmp_path / "t.tif").write_bytes(data[:-10])
    with pytest.raises(ValueError, match="truncated"):
        TiffVideo(str(tmp_path / "t.tif"))
    looped = bytearray(data)
    looped[-4:] = looped[4:8]                                 # the last directory names itself as the next
    (tmp_path / "l.tif").write_bytes(bytes(looped))
    with pytest.raises(ValueError, match="directory chain"):
        TiffVideo(str(tmp_path / "l.tif"))


def test_pages_outside_the_subset_are_pillows(tmp_path):
    """Deflate and 16 bit: opened, not native, decoded by Pillow page by page."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (2, 20, 30), dtype=np.uint8)
    path = str(tmp_path / "z.tif")
    Image.fromarray(a[0]).save(path, compression="tiff_adobe_deflate", save_all=True, append_images=[Image.fromarray(a[1])])
    from ysmr_amd.frames import TiffVideo
    video = TiffVideo(path)
    assert not video.native and video.tiff_layout_for(2) is None and video.channels == 1 and video.frame_count == 2
    np.testing.assert_array_equal(video.read(0, 2), a)
    video.close()


@pytest.mark.parametrize("name", names())
def test_read_into_equals_pillow(tmp_path, name):
    """The host path -- this reader for uncompressed strips, Pillow for the others -- delivers the recorded frames, also on a
    pool of reader threads."""
    from concurrent.futures import ThreadPoolExecutor
    _, data, frames = entry(name)
    video = opened(tmp_path, data)
    if video._compression != 1:
        pytest.importorskip("PIL.Image")
    out = np.full((len(frames) + 1,) + frames.shape[1:], 0xAA, np.uint8)
    with ThreadPoolExecutor(max_workers=3) as pool:
        assert video.read_into(0, len(frames) + 1, out, pool) == len(frames)
    np.testing.assert_array_equal(out[:-1], frames)
    assert (out[-1] == 0xAA).all()
    video.close()


def test_the_strips_as_stored(tmp_path):
    """``read_tiff_into``: the bodies back to back and the table that says where each lies and which rows it fills."""
    _, data, frames = entry("lzw_stack_3x40x52")
    video = opened(tmp_path, data)
    layout = video.tiff_layout_for(2)
    assert layout[:5] == (5, 1, 1, 16, 3)
    sizes = [int(video.strips_of(k)[1].sum()) for k in range(3)]
    assert layout[5] == max(sizes[0] + sizes[1], sizes[1] + sizes[2])
    out = np.full(layout[5] + 16, 0xAA, np.uint8)
    table = np.full((6, 5), -1, np.int32)
    n, used = video.read_tiff_into(1, 2, out[:layout[5]], table)
    assert (n, used) == (2, sizes[1] + sizes[2]) and (out[used:] == 0xAA).all()
    assert table[:, 0].tolist() == [0, 0, 0, 1, 1, 1] and table[:, 1].tolist() == [0, 16, 32] * 2 and table[:, 2].tolist() == [16, 16, 8] * 2
    for row in table:
        body = bytes(out[row[3]:row[3] + row[4]])
        status, got = tm.lzw_decode(body, int(row[2]) * 52)
        assert status == 0 and got == frames[1 + row[0], row[1]:row[1] + row[2]].tobytes()
    assert video.read_tiff_into(3, 2, out, table) == (0, 0)
    with pytest.raises(ValueError, match="the buffer"):
        video.read_tiff_into(0, 3, out[:10], np.zeros((9, 5), np.int32))
    video.close()


def test_open_video_returns_a_tiff_reader(tmp_path):
    from ysmr_amd.frames import TiffVideo, open_video
    for ext in ("x.tif", "y.TIFF"):
        path = tt.write_tiff(tmp_path / ext, [tt.page(4, 2, [bytes(range(8))])] * 2)
        video = open_video(path, default_fps=25.0)
        assert isinstance(video, TiffVideo) and video.fps == 25.0 and video.frame_count == 2
        video.close()


def test_the_decode_tiff_setting():
    from ysmr_amd import frames
    from ysmr_amd.frames import decode_tiff_setting
    assert decode_tiff_setting({}) is frames.DECODE_TIFF_DEFAULT
    assert decode_tiff_setting({"hip decode tiff": False}) is False and decode_tiff_setting({"hip decode tiff": True}) is True
    assert decode_tiff_setting({"hip decode tiff": "False"}) is False and decode_tiff_setting({"hip decode tiff": "off"}) is False
    assert decode_tiff_setting({"hip decode tiff": "true"}) is True and decode_tiff_setting({"hip decode tiff": 1}) is True
    assert decode_tiff_setting({"hip decode tiff": 0}) is False and decode_tiff_setting({"hip decode tiff": " Yes "}) is True
