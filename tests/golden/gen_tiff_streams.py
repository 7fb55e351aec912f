"""Writes ``tiff_decode_streams.npz``: TIFF files written by Pillow (its libtiff) and the frames Pillow decodes from them -- what
``TiffVideo`` delivers on the host path -- so that the GPU tests need no Pillow.

    python tests/golden/gen_tiff_streams.py          (needs Pillow built with libtiff)

The archive is written with fixed time stamps: the same Pillow gives the same bytes.  Entries: ``index`` (a JSON list of names),
``file_<name>`` (the file's bytes) and ``frames_<name>`` (u8 [T, H, W] or [T, H, W, 3] in B, G, R).
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tiff_tools as tt                                     # noqa: E402


def images():
    """name -> (frames u8 [T, H, W(, 3)] as R, G, B; Pillow's save arguments; bytes of a strip or None for libtiff's default)."""
    rng = np.random.default_rng(2024)
    uniform = rng.integers(0, 256, (96, 96), dtype=np.uint8)
    gauss = np.clip(np.rint(rng.normal(100.0, 6.0, (96, 96))), 0, 255).astype(np.uint8)
    zeros = np.zeros((300, 300), np.uint8)
    noise = rng.integers(0, 256, (40, 52), dtype=np.uint8)
    smooth = (np.add.outer(np.arange(40) * 3, np.arange(52) * 2) + rng.integers(0, 3, (40, 52))).astype(np.uint8)
    colour = np.stack([smooth, smooth[::-1], np.roll(noise // 8 + 90, 5, axis=1)], axis=2)
    rows = np.repeat((np.arange(40) * 6).astype(np.uint8)[:, None], 52, axis=1)          # constant rows: long PackBits runs
    rows[::5, 20:23] = (7, 9, 7)
    stack = np.stack([np.roll(smooth, 4 * k, axis=1) for k in range(3)])
    one = 1 << 30                                                                        # a strip size that holds any frame
    return {
        "lzw_uniform_96": (uniform[None], dict(compression="tiff_lzw"), one),
        "lzw_gauss_96": (gauss[None], dict(compression="tiff_lzw"), one),
        "lzw_zeros_300": (zeros[None], dict(compression="tiff_lzw"), one),
        "lzw_noise_40x52_rows7": (noise[None], dict(compression="tiff_lzw"), 7 * 52),
        "lzw_rgb_pred2_40x52": (colour[None], dict(compression="tiff_lzw", tiffinfo={317: 2}), 7 * 52 * 3),
        "lzw_gray_pred2_40x52": (smooth[None], dict(compression="tiff_lzw", tiffinfo={317: 2}), 16 * 52),
        "lzw_white_is_zero_40x52": (smooth[None], dict(compression="tiff_lzw", tiffinfo={262: 0}), None),
        "packbits_noise_40x52": (noise[None], dict(compression="packbits"), 16 * 52),
        "packbits_rows_40x52": (rows[None], dict(compression="packbits"), None),
        "raw_noise_40x52": (noise[None], dict(compression="raw"), 16 * 52),
        "raw_rgb_40x52": (colour[None], dict(compression="raw"), None),
        "lzw_stack_3x40x52": (stack, dict(compression="tiff_lzw"), 16 * 52),
    }


def pillow_file(frames, kw, strip_bytes):
    from PIL import Image, TiffImagePlugin
    pages = [Image.fromarray(np.ascontiguousarray(f)) for f in frames]
    before = TiffImagePlugin.STRIP_SIZE
    if strip_bytes is not None:
        TiffImagePlugin.STRIP_SIZE = strip_bytes
    try:
        buf = io.BytesIO()
        pages[0].save(buf, format="TIFF", save_all=len(pages) > 1, append_images=pages[1:], **kw)
    finally:
        TiffImagePlugin.STRIP_SIZE = before
    return buf.getvalue()


def pillow_frames(data):
    from PIL import Image
    out = []
    with Image.open(io.BytesIO(data)) as im:
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            out.append(np.asarray(im.convert("L")) if im.mode in ("L", "1") else np.asarray(im.convert("RGB"))[:, :, ::-1])
    return np.stack(out)


def big_endian_of(data):
    """The same pages in a big-endian file: the strip bodies of an 8-bit file do not depend on the byte order."""
    from PIL import Image
    pages = []
    with Image.open(io.BytesIO(data)) as im:
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            tags = im.tag_v2
            offsets, counts = tags[273], tags[279]
            pages.append(tt.page(tags[256], tags[257], [data[o:o + c] for o, c in zip(offsets, counts)], rows_per_strip=tags.get(278),
                                 compression=tags[259], photometric=tags[262], samples=tags.get(277, 1), predictor=tags.get(317, 1)))
    return tt.tiff_bytes(pages, byteorder=">", odd=True)


def files():
    out = {}
    for name, (frames, kw, strip_bytes) in images().items():
        out[name] = pillow_file(frames, kw, strip_bytes)
    out["lzw_big_endian_40x52_rows7"] = big_endian_of(out["lzw_noise_40x52_rows7"])
    return out


def write(path):
    entries, index = {}, []
    for name, data in files().items():
        index.append(name)
        entries["file_" + name] = np.frombuffer(data, np.uint8)
        entries["frames_" + name] = pillow_frames(data)
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
    target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tiff_decode_streams.npz")
    print("{}: {} files, {} bytes".format(target, write(target), os.path.getsize(target)))
