"""Writes ``mjpeg_decode_streams.npz``: JPEG streams for the Motion-JPEG decoder and, for those inside the supported subset,
the pixels Pillow decodes from them (what ``AviVideo`` delivers on the host path), so that the tests need no Pillow.

    python tests/golden/gen_mjpeg_streams.py          (needs Pillow; the recorded pixels are those of ITS libjpeg)

The archive is written with fixed time stamps: the same Pillow gives the same bytes.  Entries: ``index`` (a JSON list of
{name, height, width, sampling, status}), ``jpeg_<name>`` and, for status 0, ``pixels_<name>`` (gray [H, W] or B, G, R).
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_model as jm                                     # noqa: E402
from test_mjpeg_cpu import checkerboard, saturated          # noqa: E402

SHAPES = ((8, 8), (9, 17), (23, 41), (16, 40), (31, 33), (24, 539))
QUALITIES = (1, 50, 90, 100)
CONTENTS = ("flat", "noise", "saturated", "checkerboard")
OPTIONS = ("plain", "optimize", "rows", "blocks", "nodht")
SAMPLING_NAMES = ("L", "444", "422", "420")
UNSUPPORTED, CORRUPT = 1, 2


def content(kind, h, w, seed):
    if kind == "flat":
        return np.full((h, w, 3), (77, 130, 201), np.uint8)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "saturated":
        return saturated(h, w)
    return checkerboard(h, w)


def strip_segments(stream, marker):
    """The stream without its segments of one kind (headers only: up to SOS)."""
    out, at = bytearray(stream[:2]), 2
    while True:
        m, size = stream[at + 1], int.from_bytes(stream[at + 2:at + 4], "big")
        if m != marker:
            out += stream[at:at + 2 + size]
        at += 2 + size
        if m == 0xDA:
            return bytes(out) + stream[at:]


def pillow_stream(bgr, sampling, quality, option):
    from PIL import Image
    image = Image.fromarray(np.ascontiguousarray(bgr[..., 1])) if sampling == 0 else \
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]))
    kw = {"quality": quality}
    if sampling:
        kw["subsampling"] = sampling - 1
    if option == "optimize":
        kw["optimize"] = True
    elif option == "rows":
        kw["restart_marker_rows"] = 1
    elif option == "blocks":
        kw["restart_marker_blocks"] = 3
    elif option == "progressive":
        kw["progressive"] = True
    buf = io.BytesIO()
    image.save(buf, format="JPEG", **kw)
    stream = buf.getvalue()
    return strip_segments(stream, 0xC4) if option == "nodht" else stream


def pillow_pixels(stream, sampling):
    from PIL import Image
    with Image.open(io.BytesIO(stream)) as im:
        if sampling == 0:
            return np.asarray(im.convert("L")).copy()
        return np.asarray(im.convert("RGB"))[:, :, ::-1].copy()


def build_stream(height, width, sampling, planes, quant):
    """A baseline JPEG of given quantised coefficients (``planes[c]``: [block rows, block columns, 64] in zigzag order),
    Annex K.3 tables, no restart markers; ``quant``: one table [64] in zigzag order per component."""
    lh, lv = ((1, 1), (1, 1), (2, 1), (2, 2))[sampling]
    nc = len(planes)
    out = b"\xff\xd8"
    for c in range(nc):
        out += jm._segment(0xDB, bytes([c]) + bytes(int(v) for v in quant[c]))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([c + 1, ((lh << 4) | lv) if c == 0 else 0x11, c])
    out += jm._segment(0xC0, sof)
    for tc_th, bits, vals in ((0x00, jm.DC_LUM_BITS, jm.DC_VALS), (0x10, jm.AC_LUM_BITS, jm.AC_LUM_VALS),
                              (0x01, jm.DC_CHR_BITS, jm.DC_VALS), (0x11, jm.AC_CHR_BITS, jm.AC_CHR_VALS)):
        out += jm._segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    out += jm._segment(0xDA, sos + bytes([0, 63, 0]))
    mx, my = -(-width // (8 * lh)), -(-height // (8 * lv))
    bits, pred = jm._Bits(), [0] * nc
    for mcu in range(mx * my):
        for c in range(nc):
            h, v = (lh, lv) if c == 0 else (1, 1)
            t = min(c, 1)
            for sub in range(h * v):
                block = planes[c][(mcu // mx) * v + sub // h, (mcu % mx) * h + sub % h]
                diff = int(block[0]) - pred[c]
                pred[c] = int(block[0])
                size = jm._category(diff)
                bits.put(*jm.DC_CODES[t][size])
                if size:
                    bits.put(jm._value_bits(diff, size), size)
                run = 0
                for k in range(1, 64):
                    value = int(block[k])
                    if value == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*jm.AC_CODES[t][0xF0])
                        run -= 16
                    size = jm._category(value)
                    bits.put(*jm.AC_CODES[t][(run << 4) | size])
                    bits.put(jm._value_bits(value, size), size)
                    run = 0
                if run:
                    bits.put(*jm.AC_CODES[t][0x00])
    return out + bits.bytes_padded().replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def range_limit_stream():
    """4:2:0, 31 x 33: a few large low-frequency coefficients per block, so that many samples leave +-512, first-pass results
    leave 16 bits and (third component) dequantised coefficients do."""
    h, w = 31, 33
    rng = np.random.default_rng(11)
    mx, my = -(-w // 16), -(-h // 16)
    planes = []
    for c, (rows, cols) in enumerate(((2 * my, 2 * mx), (my, mx), (my, mx))):
        p = np.zeros((rows, cols, 64), np.int64)
        p[..., :6] = rng.integers(-400, 401, (rows, cols, 6))
        p[..., 0] = rng.integers(-1000, 1001, (rows, cols))
        planes.append(p)
    quant = [np.full(64, 8), np.full(64, 12), np.full(64, 64)]
    return h, w, build_stream(h, w, 3, planes, quant)


def streams():
    """[(name, height, width, sampling, status, stream)]"""
    out = []
    for si in range(4):
        for oi, option in enumerate(OPTIONS):
            h, w = SHAPES[(si + oi) % 6]
            quality = QUALITIES[(si + 2 * oi + oi // 2) % 4]
            kind = CONTENTS[(si + oi) % 4]
            bgr = content(kind, h, w, 17 * si + oi)
            name = "{}_{}_{}x{}_q{}_{}".format(SAMPLING_NAMES[si], option, h, w, quality, kind)
            out.append((name, h, w, si, 0, pillow_stream(bgr, si, quality, option)))
    # every quality and every content meets every sampling; the widest shape at the finest quality
    for si in range(4):
        for k in range(4):
            h, w = SHAPES[(si + k + 1) % 5]
            bgr = content(CONTENTS[k], h, w, 100 + 4 * si + k)
            name = "{}_more_{}x{}_q{}_{}".format(SAMPLING_NAMES[si], h, w, QUALITIES[(k + si) % 4], CONTENTS[k])
            out.append((name, h, w, si, 0, pillow_stream(bgr, si, QUALITIES[(k + si) % 4], "plain")))
    h, w, stream = range_limit_stream()
    out.append(("420_range_limit_31x33", h, w, 3, 0, stream))
    noise = content("noise", 23, 41, 7)
    plain = pillow_stream(noise, 1, 90, "plain")
    out.append(("444_progressive_23x41", 23, 41, 1, UNSUPPORTED, pillow_stream(noise, 1, 90, "progressive")))
    out.append(("444_app14_23x41", 23, 41, 1, UNSUPPORTED,
                plain[:2] + jm._segment(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1])) + plain[2:]))
    at = plain.index(b"\xff\xdb")
    size = int.from_bytes(plain[at + 2:at + 4], "big")
    wide = b"".join(bytes([0x10 | plain[k]]) + b"".join(bytes([0, v]) for v in plain[k + 1:k + 65])
                    for k in range(at + 4, at + 2 + size, 65))
    out.append(("444_dqt16_23x41", 23, 41, 1, UNSUPPORTED, plain[:at] + jm._segment(0xDB, wide) + plain[at + 2 + size:]))
    out.append(("444_cut_in_half_23x41", 23, 41, 1, CORRUPT, plain[:len(plain) // 2]))
    rows = pillow_stream(noise, 3, 90, "rows")
    at = rows.index(b"\xff\xd0")
    out.append(("420_rst_overwritten_23x41", 23, 41, 3, CORRUPT, rows[:at] + b"\x00\x00" + rows[at + 2:]))
    return out


def write(path):
    entries, index = {}, []
    for name, h, w, sampling, status, stream in streams():
        index.append({"name": name, "height": h, "width": w, "sampling": sampling, "status": status})
        entries["jpeg_" + name] = np.frombuffer(stream, np.uint8)
        if status == 0:
            entries["pixels_" + name] = pillow_pixels(stream, sampling)
    entries["index"] = np.frombuffer(json.dumps(index).encode(), np.uint8)
    with zipfile.ZipFile(path, "w") as archive:
        for key in sorted(entries):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(entries[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            archive.writestr(info, buf.getvalue())
    return len(index)


if __name__ == "__main__":
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mjpeg_decode_streams.npz")
    print("{}: {} streams, {} bytes".format(target, write(target), os.path.getsize(target)))
