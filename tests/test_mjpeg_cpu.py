"""The Motion-JPEG side of the annotated video without a GPU: the stream's model (tests/jpeg_model.py) against Pillow, the
structure of a stream, the writer for chunks of their own sizes, and the choice of the output format."""
import functools
import io
import os
import struct

import numpy as np
import pytest

import jpeg_model as jm

QUALITIES = (50, 90, 100)


def scene(h, w, seed=3):
    """A frame like the annotated video's: a noisy gray background, bright blobs, marks in the three colours."""
    rng = np.random.default_rng(seed)
    xx = np.arange(w)[None, :]
    gray = np.clip(60 + 20 * np.sin(xx / 7.0) + rng.normal(0, 4, (h, w)), 0, 255)
    image = np.repeat(gray[..., None], 3, axis=2).astype(np.uint8)
    image[h // 3:h // 3 + 6, w // 3:w // 3 + 6] = 230
    image[h // 2:h // 2 + 3, w - 9:w - 4] = 200
    image[5:12, 8] = (0, 255, 0)
    image[20, 10:30] = (15, 165, 253)
    image[28:31, 40:43] = (255, 255, 255)
    return image


def saturated(h, w, seed=5):
    """0 / 255 only: whole blocks of one value beside each other (the largest DC differences), then single pixels."""
    rng = np.random.default_rng(seed)
    image = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    for k in range(3):
        image[:8, 8 * k:8 * k + 8] = 255 * (k & 1)
        image[8:16, 8 * k:8 * k + 8] = 255 * (~k & 1)
    return image


def checkerboard(h, w):
    """Pixels alternately 118 and 138: at quality 50 only the last coefficient of the zigzag sequence survives the
    quantisation, behind a run of 62 zeros (three ZRL codes).  (At full contrast every odd-odd coefficient survives, and
    the runs between them are short.)"""
    yy, xx = np.mgrid[:h, :w]
    return np.repeat((118 + ((yy + xx) & 1) * 20).astype(np.uint8)[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def images():
    rng = np.random.default_rng(0)
    out = {"scene37x50": scene(37, 50), "noise23x41": rng.integers(0, 256, (23, 41, 3), dtype=np.uint8),
           "saturated16x40": saturated(16, 40), "flat8x8": np.full((8, 8, 3), 77, np.uint8)}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def encoded(name, quality):
    return jm.encode_info(images()[name], quality)


def _psnr(a, b):
    err = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if err == 0 else 10 * np.log10(255.0 ** 2 / err)


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("name", ["scene37x50", "noise23x41", "saturated16x40", "flat8x8"])
def test_the_model_writes_a_jpeg_as_good_as_pillows(name, quality):
    Image = pytest.importorskip("PIL.Image")
    bgr = images()[name]
    stream, _ = encoded(name, quality)
    mine = Image.open(io.BytesIO(stream))
    mine.load()
    assert mine.size == (bgr.shape[1], bgr.shape[0]) and mine.mode == "RGB" and mine.format == "JPEG"
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, format="JPEG", quality=quality, subsampling=0)
    theirs = Image.open(io.BytesIO(buf.getvalue()))
    theirs.load()
    assert mine.quantization == theirs.quantization
    p_mine, p_theirs = _psnr(np.asarray(mine)[..., ::-1], bgr), _psnr(np.asarray(theirs)[..., ::-1], bgr)
    print("{} q{}: PSNR model {:.2f} dB, Pillow {:.2f} dB; {} bytes against {}".format(
        name, quality, p_mine, p_theirs, len(stream), len(buf.getvalue())))
    assert p_mine >= p_theirs - 0.5
    if bgr.shape[0] * bgr.shape[1] >= 37 * 50:
        assert len(stream) <= 1.05 * len(buf.getvalue())


def _segments(stream):
    """[(marker, body)] up to and including SOS, and the entropy-coded data with its RST markers, without EOI."""
    assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
    at, found = 2, [(0xD8, b"")]
    while True:
        assert stream[at] == 0xFF
        marker, size = stream[at + 1], struct.unpack(">H", stream[at + 2:at + 4])[0]
        found.append((marker, stream[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xDA:
            return found, stream[at:-2]


def test_structure_of_a_stream_of_three_mcu_rows():
    bgr = np.ascontiguousarray(np.tile(images()["noise23x41"], (1, 1, 1))[:20, :29])      # 3 MCU rows of 4
    stream, info = jm.encode_info(bgr, 100)
    found, data = _segments(stream)
    assert [m for m, _ in found] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    body = dict((m, b) for m, b in found if m != 0xC4)
    assert body[0xE0] == b"AVI1" + bytes(10)
    assert len(body[0xDB]) == 130 and body[0xDB][0] == 0 and body[0xDB][65] == 1
    assert body[0xC0] == bytes([8, 0, 20, 0, 29, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [b[0] for m, b in found if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    assert struct.unpack(">H", body[0xDD])[0] == 4 == (29 + 7) // 8
    assert body[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(jm.header(20, 29, 100)) == 625 and stream.startswith(jm.header(20, 29, 100))
    # the data: interval, RST0, interval, RST1, interval; every other 0xFF is followed by 0x00
    sizes = info["interval_bytes"]
    assert len(sizes) == 3 and len(data) == sum(sizes) + 4
    assert data[sizes[0]:sizes[0] + 2] == b"\xff\xd0"
    assert data[sizes[0] + 2 + sizes[1]:sizes[0] + 4 + sizes[1]] == b"\xff\xd1"
    markers = {sizes[0], sizes[0] + 2 + sizes[1]}
    seen_ff = 0
    for at in range(len(data)):
        if data[at] == 0xFF and at not in markers:
            assert at + 1 < len(data) and data[at + 1] == 0x00, "0xFF at {} followed by {:#x}".format(at, data[at + 1])
            seen_ff += 1
    assert seen_ff == info["stuffed"] > 0


def test_the_case_set_reaches_the_hard_codes():
    """What the byte-for-byte tests on the device lean on: stuffed bytes, ZRL codes and the largest DC category all occur."""
    infos = [encoded(name, q)[1] for name in images() for q in QUALITIES]
    infos.append(jm.encode_info(checkerboard(16, 24), 50)[1])
    assert infos[-1]["zrl"] > 0
    assert encoded("saturated16x40", 100)[1]["max_dc_category"] == 11
    assert max(i["max_category"] for i in infos) == 11
    assert sum(i["stuffed"] for i in infos) > 0 and sum(i["zrl"] for i in infos) > 0
    assert all(sum(i["interval_bytes"]) > 0 for i in infos)


def test_huffman_tables_are_the_ones_pillow_writes():
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, format="JPEG", quality=90, subsampling=0)
    theirs = sorted(b for m, b in _segments_all(buf.getvalue()) if m == 0xC4)
    mine = sorted(b for m, b in _segments(jm.encode(np.zeros((8, 8, 3), np.uint8), 90))[0] if m == 0xC4)
    assert b"".join(mine) == b"".join(_split_dht(b"".join(theirs)))


def _segments_all(stream):
    at, found = 2, []
    while stream[at + 1] != 0xDA:
        size = struct.unpack(">H", stream[at + 2:at + 4])[0]
        found.append((stream[at + 1], stream[at + 4:at + 2 + size]))
        at += 2 + size
    return found


def _split_dht(body):
    """The tables of DHT bodies that may hold several each, sorted as single-table bodies."""
    at, tables = 0, []
    while at < len(body):
        n = sum(body[at + 1:at + 17])
        tables.append(body[at:at + 17 + n])
        at += 17 + n
    return sorted(tables)


# ---- the writer ----------------------------------------------------------------------------------------------------------

def _walk(data, at, end):
    """[(id, payload offset, size)] of the chunks in data[at:end]; a LIST gives ('LIST:kind', ...) and its children follow."""
    found = []
    while at < end:
        cid, size = struct.unpack_from("<4sI", data, at)
        if cid in (b"RIFF", b"LIST"):
            found.append((cid.decode() + ":" + data[at + 8:at + 12].decode(), at + 12, size - 4))
            found += _walk(data, at + 12, at + 8 + size)
        else:
            found.append((cid.decode(), at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end, "chunks overrun their parent: {} != {}".format(at, end)
    return found


def _blobs(n=5):
    """JPEGs of different, partly odd sizes, as chunks back to back."""
    rng = np.random.default_rng(7)
    jpegs = [jm.encode(rng.integers(0, 256, (9, 13, 3), dtype=np.uint8), q) for q in (30, 55, 80, 90, 100)[:n]]
    k = 0
    while all(len(j) % 2 == 0 for j in jpegs) or all(len(j) % 2 for j in jpegs):      # both parities must occur
        k += 1
        jpegs[0] = jm.encode(rng.integers(0, 256, (9, 13, 3), dtype=np.uint8), 30 + k)
    chunks = [jm.chunk(j) for j in jpegs]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
    return jpegs, np.frombuffer(b"".join(chunks), np.uint8), offsets


@pytest.mark.parametrize("riff_limit", [1 << 30, 4000])
def test_writer_of_chunks_with_their_own_sizes(tmp_path, riff_limit):
    from ysmr_amd.annotate import AviWriter, MjpegAviWriter
    jpegs, data, offsets = _blobs()
    assert len({len(j) for j in jpegs}) == 5
    path = str(tmp_path / "m.avi")
    w = MjpegAviWriter(path, 13, 9, 29.97002997, riff_limit=riff_limit)
    w.write_chunks(data[:offsets[2]], offsets[:3])                 # two calls: a run may end anywhere
    w.write_chunks(data[offsets[2]:], offsets[2:] - offsets[2])
    w.close()
    raw = open(path, "rb").read()
    tree = _walk(raw, 0, len(raw))
    riffs = [t for t in tree if t[0].startswith("RIFF")]
    assert riffs[0][0] == "RIFF:AVI " and all(t[0] == "RIFF:AVIX" for t in riffs[1:])
    assert (len(riffs) > 1) == (riff_limit == 4000)
    assert sum(t[2] + 12 for t in riffs) == len(raw)               # the RIFF sizes cover the file
    assert all(t[2] + 12 <= riff_limit for t in riffs)
    frames = [t for t in tree if t[0] == "00dc"]
    assert [raw[o:o + s] for _, o, s in frames] == jpegs
    for (_, o, s), j in zip(frames, jpegs):
        if s & 1:
            assert raw[o + s] == 0                                   # the pad byte
    body = {t[0]: raw[t[1]:t[1] + t[2]] for t in tree if t[0] in ("avih", "strh", "strf", "dmlh", "idx1")}
    first = [t for t in frames if t[1] < riffs[0][1] + riffs[0][2]]
    avih = struct.unpack("<14I", body["avih"])
    assert avih[4] == len(first) and avih[7] == max(len(j) for j in jpegs) and avih[8:10] == (13, 9)
    strh = struct.unpack("<4s4sIHHIIIIIIiI4h", body["strh"])
    assert strh[:2] == (b"vids", b"MJPG") and (strh[6], strh[7]) == (1001, 30000) and strh[9] == 5
    assert strh[10] == max(len(j) for j in jpegs)
    strf = struct.unpack("<IiiHHIIiiII", body["strf"])
    assert strf[:7] == (40, 13, 9, 1, 24, struct.unpack("<I", b"MJPG")[0], max(len(j) for j in jpegs))
    assert struct.unpack("<I", body["dmlh"])[0] == 5
    movi = next(t for t in tree if t[0] == "LIST:movi")
    entries = [struct.unpack_from("<4sIII", body["idx1"], 16 * k) for k in range(len(body["idx1"]) // 16)]
    assert len(entries) == len(first)
    for (cid, flags, off, size), (_, o, s) in zip(entries, first):
        assert (cid, flags, size) == (b"00dc", 0x10, s) and movi[1] - 4 + off == o - 8
    assert AviWriter.HEADER_BYTES == movi[1]


def test_written_file_is_read_back_frame_for_frame(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ysmr_amd.annotate import MjpegAviWriter
    from ysmr_amd.frames import AviVideo
    jpegs, data, offsets = _blobs()
    for riff_limit in (1 << 30, 4000):
        path = str(tmp_path / "m{}.avi".format(riff_limit))
        w = MjpegAviWriter(path, 13, 9, 25.0, riff_limit=riff_limit)
        w.write_chunks(data, offsets)
        w.close()
        video = AviVideo(path)
        assert (video.frame_count, video.frames_available, video.height, video.width, video.fps) == (5, 5, 9, 13, 25.0)
        got = video.read(0, 5)
        video.close()
        for k, j in enumerate(jpegs):
            want = np.asarray(Image.open(io.BytesIO(j)).convert("RGB"))[..., ::-1]
            assert np.array_equal(np.asarray(got[k]).reshape(want.shape), want), "frame {}".format(k)


def test_writer_refuses_what_is_not_a_run_of_chunks(tmp_path):
    from ysmr_amd.annotate import MjpegAviWriter
    _, data, offsets = _blobs()
    w = MjpegAviWriter(str(tmp_path / "m.avi"), 13, 9, 25.0)
    with pytest.raises(ValueError):
        w.write_chunks(data, offsets + 1)
    with pytest.raises(ValueError):
        w.write_chunks(data[:-1], offsets)
    with pytest.raises(ValueError):
        w.write_chunks(data.reshape(1, -1), offsets)
    w.abort()
    assert not os.path.exists(str(tmp_path / "m.avi"))


# ---- the choice of the format --------------------------------------------------------------------------------------------

def test_output_format():
    from ysmr_amd.annotate import output_format
    from ysmr_amd.helper_file import default_settings
    fmt, quality, warning = output_format(default_settings())                          # .mp4 / mp4v
    assert fmt == "raw" and "the HIP path has no encoder; writing an uncompressed 24-bit AVI instead" in warning
    assert "'.mp4'" in warning and "'mp4v'" in warning

    def asked(ext, codec, **more):
        return output_format(default_settings(**{"save video file extension": ext, "save video fourcc codec": codec, **more}))

    assert asked(".avi", "DIB ") == ("raw", None, None)
    for codec in ("mjpg", "MJPG", "JPEG", "Jpeg"):
        assert asked(".avi", codec) == ("mjpeg", 90, None)
        assert asked(".AVI", codec) == ("mjpeg", 90, None)
    assert asked(".avi", "MJPG", **{"hip video jpeg quality": 50}) == ("mjpeg", 50, None)
    assert asked(".avi", "MJPG", **{"hip video jpeg quality": "100"}) == ("mjpeg", 100, None)
    assert asked(".avi", "MJPG", **{"hip video jpeg quality": 1}) == ("mjpeg", 1, None)
    for bad in (0, 101, -5, "many"):
        with pytest.raises(ValueError, match="hip video jpeg quality"):
            asked(".avi", "MJPG", **{"hip video jpeg quality": bad})
    fmt, quality, warning = asked(".mp4", "MJPG")
    assert fmt == "raw" and "no encoder" in warning
    fmt, quality, warning = asked(".avi", "XVID", **{"hip video jpeg quality": 0})     # (only Motion-JPEG reads the key)
    assert fmt == "raw" and "no encoder" in warning


def test_a_bad_quality_is_refused_before_any_frame(tmp_path, caplog):
    from ysmr_amd import annotate_video
    from ysmr_amd.helper_file import default_settings
    import pandas as pd
    path = str(tmp_path / "clip.npy")
    np.save(path, np.zeros((2, 16, 16), np.uint8))
    s = default_settings(**{"log to file": False, "save video file extension": ".avi", "save video fourcc codec": "MJPG",
                            "hip video jpeg quality": 101})
    df = pd.DataFrame({"TRACK_ID": [1], "POSITION_T": [0], "POSITION_X": [3.0], "POSITION_Y": [3.0], "moving": [1],
                       "turn_points": [0], "motility_phenotype": [2]})
    assert annotate_video(path, df, settings=s, result_folder=str(tmp_path / "out")) is None
    assert "hip video jpeg quality" in caplog.text
    assert not os.path.exists(str(tmp_path / "out" / "clip_annotated_output.avi"))


def test_mjpeg_entry_points_refuse_bad_arguments_without_a_gpu():
    from ysmr_amd import _lib
    L = _lib.lib()
    assert L.ysmr_mjpeg_workspace_bytes(2, 16, 24) >= 2 * 2 * 3 * 3 * (128 + 208)
    assert L.ysmr_mjpeg_workspace_bytes(0, 16, 24) == 0 and L.ysmr_mjpeg_workspace_bytes(1, 70000, 24) == 0
    ws = L.ysmr_mjpeg_workspace_bytes(1, 16, 24)
    good = dict(stream=None, dib=256, n=1, h=16, w=24, stride=72, frame_bytes=72 * 16, bottom_up=1, quality=90, ws=512,
                ws_bytes=ws, out=1024, cap=100, offsets=2048, status=4096)

    def call(**change):
        a = dict(good, **change)
        return L.ysmr_mjpeg_batch(a["stream"], a["dib"], a["n"], a["h"], a["w"], a["stride"], a["frame_bytes"], a["bottom_up"],
                                  a["quality"], a["ws"], a["ws_bytes"], a["out"], a["cap"], a["offsets"], a["status"])

    for change in (dict(dib=None), dict(ws=None), dict(out=None), dict(offsets=None), dict(status=None), dict(quality=0),
                   dict(quality=101), dict(stride=71), dict(stride=70), dict(stride=68), dict(frame_bytes=72 * 16 - 1),
                   dict(ws_bytes=ws - 1), dict(n=0), dict(h=0), dict(w=0), dict(ws=520)):
        assert call(**change) == _lib.YSMR_ERR_ARG, change
        assert L.ysmr_last_error()
