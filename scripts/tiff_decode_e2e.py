"""track_bacteria end to end from TIFF stacks of the bench clip (S500, 1228 x 922, 1920 frames), decoded on the device ('hip decode
tiff' True: the stored strips cross the bus, ysmr_tiff_decode_batch decodes them) against the host path (False: uncompressed strips
read directly, compressed ones by Pillow on the feed's reader threads).  One warm process; the two paths alternate.

  python3 scripts/tiff_decode_e2e.py [FRAMES [DIR]]

The clip is saved in six ways -- uncompressed TIFF, LZW with libtiff's default strips, LZW with predictor 2, LZW with one strip per
frame, PackBits, and .npy as the ceiling -- by Pillow (its libtiff), a page per call on 16 threads, chained into a stack here.  Per file: the stored bytes per frame, the decode call alone per batch (events), and frames/s of
track_bacteria on either path, three warm runs each with their range.  The output belongs in profiles/tiff_decode_e2e.log."""
import io
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HEIGHT, WIDTH, BLOBS, FRAMES, BATCH = 922, 1228, 500, 1920, 64
VARIANTS = (("raw.tif", dict(compression="raw"), None),
            ("lzw.tif", dict(compression="tiff_lzw"), None),
            ("lzw_pred2.tif", dict(compression="tiff_lzw", tiffinfo={317: 2}), None),
            ("lzw_one_strip.tif", dict(compression="tiff_lzw"), 1 << 30),
            ("packbits.tif", dict(compression="packbits"), None))


def settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False})
    s.update(kw)
    return s


def write_stack(path, clip, kw, strip_bytes):
    """The clip as a multi-page TIFF: every page encoded by Pillow on its own, the pages chained here."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image, TiffImagePlugin
    import tiff_tools as tt
    before = TiffImagePlugin.STRIP_SIZE
    if strip_bytes is not None:
        TiffImagePlugin.STRIP_SIZE = strip_bytes

    def one(frame):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, format="TIFF", **kw)
        data = buf.getvalue()
        with Image.open(io.BytesIO(data)) as im:
            tags = im.tag_v2
            bodies = [data[o:o + c] for o, c in zip(tags[273], tags[279])]
            return tt.page(tags[256], tags[257], bodies, rows_per_strip=tags.get(278), compression=tags[259], photometric=tags[262],
                           predictor=tags.get(317, 1))

    def long_values(fh, values):
        """An entry's value field for LONGs: the value itself, or where the values were written."""
        if len(values) == 1:
            return struct.pack("<I", values[0])
        where = fh.tell()
        fh.write(struct.pack("<{}I".format(len(values)), *values))
        return struct.pack("<I", where)

    try:
        with ThreadPoolExecutor(16) as pool, open(path, "wb") as fh:
            fh.write(b"II" + struct.pack("<HI", 42, 0))
            link = 4
            for page in pool.map(one, clip):
                offsets = []
                for body in page["bodies"]:                          # as libtiff lays them out: back to back, odd offsets too
                    offsets.append(fh.tell())
                    fh.write(body)
                if fh.tell() & 1:
                    fh.write(b"\0")
                entries = {256: (4, 1, struct.pack("<I", page["width"])), 257: (4, 1, struct.pack("<I", page["height"])),
                           258: (3, 1, struct.pack("<HH", 8, 0)), 259: (3, 1, struct.pack("<HH", page["compression"], 0)),
                           262: (3, 1, struct.pack("<HH", page["photometric"], 0)), 273: (4, len(offsets), long_values(fh, offsets)),
                           277: (3, 1, struct.pack("<HH", 1, 0)), 278: (4, 1, struct.pack("<I", page["rows_per_strip"] or page["height"])),
                           279: (4, len(offsets), long_values(fh, [len(b) for b in page["bodies"]]))}
                if page["predictor"] != 1:
                    entries[317] = (3, 1, struct.pack("<HH", page["predictor"], 0))
                ifd = fh.tell()
                fh.write(struct.pack("<H", len(entries)))
                for tag in sorted(entries):
                    kind, n, value = entries[tag]
                    fh.write(struct.pack("<HHI", tag, kind, n) + value)
                fh.write(struct.pack("<I", 0))
                end = fh.tell()
                fh.seek(link)
                fh.write(struct.pack("<I", ifd))
                fh.seek(end)
                link = end - 4
    finally:
        TiffImagePlugin.STRIP_SIZE = before


def make(folder, frames):
    from ysmr_amd.synth import SyntheticVideo
    clip = SyntheticVideo(HEIGHT, WIDTH, BLOBS, seed=0).frames(frames)
    np.save(os.path.join(folder, "clip.npy"), clip)
    for name, kw, strip_bytes in VARIANTS:
        t0 = time.perf_counter()
        write_stack(os.path.join(folder, name), clip, kw, strip_bytes)
        print("{}: written in {:.1f} s".format(name, time.perf_counter() - t0), flush=True)
    return clip


def decode_call(path, repeats=5):
    """ysmr_tiff_decode_batch alone on the first batch of the file: milliseconds per batch by events."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.frames import TiffVideo
    video = TiffVideo(path)
    layout = video.tiff_layout_for(BATCH)
    stored = sum(int(video.strips_of(k)[1].sum()) for k in range(video.frame_count)) / video.frame_count
    print("{}: {:.0f} KB stored per frame, {} strips per frame of {} rows, tiff_layout_for({}) {}".format(
        os.path.basename(path), stored / 1e3, video._strips_per_frame, video._rows_per_strip, BATCH, layout), flush=True)
    if layout is None:
        video.close()
        return
    compression, predictor, photometric, rows_per_strip, spf, most = layout
    n = min(BATCH, video.frame_count)
    host, table = np.empty(most, np.uint8), np.zeros((n * spf, 5), np.int32)
    assert video.read_tiff_into(0, n, host, table)[0] == n
    L = _lib.lib()
    bodies, strips = torch.from_numpy(host).cuda(), torch.from_numpy(table).cuda()
    ws_bytes = L.ysmr_tiff_decode_workspace_bytes(n, video.height, video.width, video.channels, compression, predictor, photometric,
                                                  rows_per_strip, most)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, video.height, video.width), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    times = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.ysmr_tiff_decode_batch(None, bodies.data_ptr(), strips.data_ptr(), n * spf, n, video.height, video.width,
                                            video.channels, compression, predictor, photometric, ws.data_ptr(), ws_bytes, out.data_ptr(),
                                            status.data_ptr()), "ysmr_tiff_decode_batch")
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    assert not status.any().item(), "a frame was flagged"
    assert np.array_equal(out[:2].cpu().numpy(), video.read(0, 2)), "the device and the host path disagree"
    print("{}: ysmr_tiff_decode_batch, {} frames: {} ms, median {:.2f} ms = {:.0f} frames/s".format(
        os.path.basename(path), n, " ".join("{:.2f}".format(t) for t in times[1:]), statistics.median(times[1:]),
        n / statistics.median(times[1:]) * 1e3), flush=True)
    video.close()


def run(path, reps=3):
    import torch
    from ysmr_amd.frames import open_video
    from ysmr_amd.track_eval import track_bacteria
    video = open_video(path)
    frames = getattr(video, "frames_available", video.frame_count)
    video.close()
    modes = (True, False) if path.endswith(".tif") else (True,)
    out = tempfile.mkdtemp(prefix="tiff_decode_e2e_")
    rates, rows = {m: [] for m in modes}, {}
    try:
        for rep in range(reps + 1):                                  # (the first round warms up: library, allocator, page cache)
            for on_device in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = track_bacteria(path, settings=settings(**{"hip decode tiff": on_device}), result_folder=out)
                dt = time.perf_counter() - t0
                rows[on_device] = len(res[0])
                if rep:
                    rates[on_device].append(frames / dt)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    name = os.path.basename(path)
    for on_device in modes:
        label = "'hip decode tiff' {}".format(on_device) if path.endswith(".tif") else "(no decode)"
        print("{}: {}: {} frames/s, range {:.0f} .. {:.0f}, median {:.0f} ({} rows)".format(
            name, label, " ".join("{:.0f}".format(r) for r in rates[on_device]), min(rates[on_device]), max(rates[on_device]),
            statistics.median(rates[on_device]), rows[on_device]), flush=True)
    assert len(set(rows.values())) == 1, "the two paths tracked different tables"
    return rates


if __name__ == "__main__":
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else FRAMES
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="tiff_decode_e2e_")
    os.makedirs(work, exist_ok=True)
    try:
        make(work, n_frames)
        rates = {}
        for name in [v[0] for v in VARIANTS]:
            decode_call(os.path.join(work, name))
        for name in [v[0] for v in VARIANTS] + ["clip.npy"]:
            rates[name] = run(os.path.join(work, name))
        lzw = rates["lzw.tif"]
        print("rule for the default (lzw.tif): device {:.0f} .. {:.0f}, host {:.0f} .. {:.0f}: 'hip decode tiff' defaults to {}".format(
            min(lzw[True]), max(lzw[True]), min(lzw[False]), max(lzw[False]), min(lzw[True]) > max(lzw[False])))
    finally:
        if len(sys.argv) <= 2:
            shutil.rmtree(work, ignore_errors=True)
