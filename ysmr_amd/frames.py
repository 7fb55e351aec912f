"""Frame sources for the detect-and-link path.

The reference reads frames with ``cv2.VideoCapture`` (ysmr/track_eval.py:65-93, 159).  OpenCV is
not a dependency of this package, so raw containers are read natively and ``cv2`` is used only when
it happens to be importable:

* ``.npy``  -- uint8 array [T, H, W] (gray) or [T, H, W, 3] (BGR), memory-mapped; fps from a
               ``<name>_meta.json`` side file (key ``fps``) or the tracking.ini value
* ``.y4m``  -- YUV4MPEG2; the luma plane is used as the gray frame
* ``.avi``  -- uncompressed AVI (what many microscope cameras write): 8-bit gray or 24-bit BGR DIB frames,
               bottom-up or top-down, OpenDML ``AVIX`` extensions included -- ``DeviceFrameFeed`` uploads the stored
               frames as they are and unpacks them on the device (``ysmr_unpack_dib_batch``); Motion-JPEG AVI: baseline
               frames (gray, 4:4:4, 4:2:2, 4:2:0) are uploaded as they are and decoded on the device
               (``ysmr_mjpeg_decode_batch``), anything else by Pillow on the reader threads, if it can be imported; other
               compressed streams go to cv2
* ``.tif`` / ``.tiff`` -- multi-page TIFF stack, a page per frame (``TiffVideo``): 8-bit gray or RGB strips, uncompressed,
               LZW (with or without the horizontal predictor) or PackBits, are uploaded as stored and decoded on the device
               (``ysmr_tiff_decode_batch``); other pages by Pillow, if it can be imported; fps from the tracking.ini value
* anything else -- ``cv2.VideoCapture`` if cv2 can be imported, otherwise an error

Every source exposes ``frame_count`` (what the container reports: cv2's CAP_PROP_FRAME_COUNT), optionally
``frames_available`` (what it holds, when that can differ), ``fps``, ``height``, ``width``, ``channels`` and
``read(start, count) -> uint8 ndarray [n, H, W(, 3)]`` (fewer than ``count`` frames at the end).
"""
from __future__ import annotations

import json
import os

import numpy as np

__all__ = ["open_video", "NpyVideo", "Y4mVideo", "AviVideo", "TiffVideo", "Cv2Video", "DeviceFrameFeed"]


class NpyVideo:
    def __init__(self, path, default_fps=30.0):
        self.path = path
        self._a = np.load(path, mmap_mode="r")
        if self._a.dtype != np.uint8 or self._a.ndim not in (3, 4):
            raise ValueError(f"{path}: expected uint8 [T,H,W] or [T,H,W,3], got {self._a.dtype} {self._a.shape}")
        if self._a.ndim == 4 and self._a.shape[3] != 3:
            raise ValueError(f"{path}: colour frames must have 3 channels")
        self.frame_count, self.height, self.width = (int(v) for v in self._a.shape[:3])
        self.channels = 1 if self._a.ndim == 3 else 3
        self.fps = float(default_fps)
        # positional reads for read_into: where the frames start in the file, and a descriptor of its own
        self._data0 = int(getattr(self._a, "offset", 0)) if self._a.flags["C_CONTIGUOUS"] else None
        self._fd = os.open(path, os.O_RDONLY) if self._data0 is not None else None
        meta = os.path.splitext(path)[0] + "_meta.json"
        try:
            with open(meta) as fh:
                self.fps = float(json.load(fh).get("fps", self.fps))
        except (OSError, ValueError, TypeError):
            pass

    def read(self, start, count):
        return np.ascontiguousarray(self._a[start:start + count])

    def read_into(self, start, count, out, pool=None):
        """Copy frames [start, start + count) into ``out[:n]`` (any writable uint8 array of the frame shape, e.g. pinned
        memory).  Positional reads side by side in ONE native call (``ysmr_file_read``, as many threads as the pool has, no
        Python between the pieces): the kernel copies page-cache pages straight into ``out``.  (Copying out of the memory map faults every 4-KiB page in first, and the faults of all
        threads queue on the one address space: 36 GB/s whatever the number of threads, which was the frame loop of
        ``track_bacteria``.)"""
        n = max(0, min(count, self.frame_count - start))
        if n == 0:
            return 0
        dst = out[:n]
        if self._fd is None or not dst.flags["C_CONTIGUOUS"]:
            np.copyto(dst, self._a[start:start + n])
            return n
        frame_bytes = self.height * self.width * self.channels
        threads = 1 if pool is None else pool._max_workers
        from . import _lib
        _lib.check(_lib.lib().ysmr_file_read(self._fd, dst.ctypes.data, n * frame_bytes, self._data0 + start * frame_bytes, threads),
                   "ysmr_file_read")
        return n

    def close(self):
        self._a = None
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None


class Y4mVideo:
    """Minimal YUV4MPEG2 reader (8-bit; C420*, C422, C444 or Cmono): luma only."""

    def __init__(self, path, default_fps=30.0):
        self.path = path
        self._fh = open(path, "rb")
        header = self._fh.readline()
        if not header.startswith(b"YUV4MPEG2"):
            raise ValueError(f"{path}: not a YUV4MPEG2 file")
        self.fps, chroma = float(default_fps), "420"
        for tok in header.split()[1:]:
            t = tok.decode("ascii", "replace")
            if t[0] == "W":
                self.width = int(t[1:])
            elif t[0] == "H":
                self.height = int(t[1:])
            elif t[0] == "F" and ":" in t:
                num, den = t[1:].split(":")
                if int(den):
                    self.fps = int(num) / int(den)
            elif t[0] == "C":
                chroma = t[1:]
        y = self.width * self.height
        if chroma.startswith("420"):
            cw, ch = (self.width + 1) // 2, (self.height + 1) // 2
            self._frame_bytes = y + 2 * cw * ch
        elif chroma.startswith("422"):
            self._frame_bytes = y + 2 * ((self.width + 1) // 2) * self.height
        elif chroma.startswith("444"):
            self._frame_bytes = 3 * y
        elif chroma.startswith("mono"):
            self._frame_bytes = y
        else:
            raise ValueError(f"{path}: unsupported chroma '{chroma}'")
        self._data0 = self._fh.tell()
        size = os.path.getsize(path) - self._data0
        self._stride = len(b"FRAME\n") + self._frame_bytes   # frames without per-frame parameters
        self.frame_count = size // self._stride
        self.channels = 1

    def read(self, start, count):
        n = max(0, min(count, self.frame_count - start))
        out = np.empty((n, self.height, self.width), np.uint8)
        self.read_into(start, n, out)
        return out

    def read_into(self, start, count, out, pool=None):
        """Luma planes of frames [start, start + count) straight into ``out[:n]`` (e.g. pinned memory)."""
        n = max(0, min(count, self.frame_count - start))
        for i in range(n):
            self._fh.seek(self._data0 + (start + i) * self._stride)
            marker = self._fh.readline()
            if not marker.startswith(b"FRAME"):
                raise ValueError(f"{self.path}: frame {start + i} has no FRAME marker")
            plane = memoryview(out[i]).cast("B")
            if self._fh.readinto(plane) != self.width * self.height:
                raise ValueError(f"{self.path}: frame {start + i} is truncated")
        return n

    def close(self):
        self._fh.close()


class AviVideo:
    """AVI (RIFF) without OpenCV: stream 0 must be video with BI_RGB 8- or 24-bit frames (or the raw
    gray fourccs Y800 / GREY / Y8), or Motion-JPEG (``jpeg_layout``: decoded on the device; else with Pillow, if installed).  8-bit frames whose palette is the gray ramp are delivered as gray
    [H, W] -- what ``cv2.VideoCapture`` + ``COLOR_BGR2GRAY`` make of them --, other palettes are
    expanded to BGR; 24-bit frames are BGR as stored.  Raises ValueError for compressed streams."""

    _RAW_GRAY = (b"Y800", b"GREY", b"Y8  ")

    def __init__(self, path, default_fps=30.0):
        self.path = path
        self._fh = open(path, "rb")
        try:
            self._parse(path, default_fps)
        except BaseException:
            self._fh.close()           # (open_video falls through to OpenCV on ValueError: do not leak the handle)
            raise

    def _parse(self, path, default_fps):
        import struct
        fh = self._fh
        size = os.path.getsize(path)
        self.fps = float(default_fps)
        self._frames = []          # (offset, size) of every video chunk of stream 0
        declared = [0]
        bih = palette = None
        first_stream = True

        def walk(start, end, depth):
            nonlocal bih, palette, first_stream
            pos = start
            while pos + 8 <= end:
                fh.seek(pos)
                cid, csz = struct.unpack("<4sI", fh.read(8))
                body = pos + 8
                if cid in (b"RIFF", b"LIST"):
                    kind = fh.read(4)
                    if kind == b"movi":
                        walk_movi(body + 4, min(body + csz, end))
                    elif kind in (b"AVI ", b"AVIX", b"hdrl", b"strl"):
                        walk(body + 4, min(body + csz, end), depth + 1)
                elif cid == b"strh":
                    data = fh.read(min(csz, 56))
                    if first_stream and data[:4] == b"vids" and len(data) >= 28:
                        scale, rate = struct.unpack("<II", data[20:28])
                        if scale and rate:
                            self.fps = rate / scale
                        if len(data) >= 36:
                            declared[0] = struct.unpack("<I", data[32:36])[0]     # dwLength: the stream's frames
                elif cid == b"strf" and first_stream:
                    data = fh.read(csz)
                    if len(data) >= 40:
                        bih = struct.unpack("<IiiHHIIiiII", data[:40])
                        palette = data[40:]
                    first_stream = False
                pos = body + csz + (csz & 1)

        def walk_movi(start, end):
            pos = start
            while pos + 8 <= end:
                fh.seek(pos)
                cid, csz = struct.unpack("<4sI", fh.read(8))
                body = pos + 8
                if cid == b"LIST":                       # 'rec ' groups
                    walk_movi(body + 4, min(body + csz, end))
                elif cid[:2] == b"00" and cid[2:] in (b"db", b"dc"):
                    # an EMPTY chunk is AVI's "frame dropped by the capture, show the previous one again":
                    # it still occupies a frame slot (cv2.VideoCapture delivers the repeated frame, so
                    # POSITION_T and the frame count stay aligned with the reference)
                    if csz:
                        self._frames.append((body, csz))
                    elif self._frames:
                        self._frames.append(self._frames[-1])
                pos = body + csz + (csz & 1)

        if fh.read(4) != b"RIFF":
            raise ValueError(f"{path}: not a RIFF file")
        walk(0, size, 0)
        if bih is None:
            raise ValueError(f"{path}: no video stream format found")
        _, width, height, _, bits, compression, *_ = bih
        fourcc = struct.pack("<I", compression)
        self._jpeg = fourcc.upper() in (b"MJPG", b"JPEG")
        if self._jpeg:
            try:
                from PIL import Image
                self._Image, self._no_pillow = Image, None
            except ImportError as exc:
                self._Image, self._no_pillow = None, str(exc)
            self.width, self.height = int(width), abs(int(height))
            self.frames_available = len(self._frames)
            self.frame_count = declared[0] or self.frames_available
            if not self.frames_available:
                raise ValueError(f"{path}: no frames")
            # the first frame's SOF / SOS say what the file holds: Pillow is needed only for frames the device does not decode
            components, self._jpeg_sampling, self._jpeg_dri = self._jpeg_first(self._chunk(0).getvalue())
            if self.jpeg_layout_for(1) is None and self._Image is None:
                raise ValueError(f"{path}: Motion-JPEG AVI needs Pillow ({self._no_pillow})")
            if components is None:
                with self._Image.open(self._chunk(0)) as first:
                    components = 1 if first.mode == "L" else 3
            self.channels = 1 if components == 1 else 3
            return
        if not (compression == 0 or (fourcc in self._RAW_GRAY and bits == 8)) or bits not in (8, 24):
            raise ValueError(f"{path}: only uncompressed 8/24-bit or Motion-JPEG AVI is read natively "
                             f"(fourcc {fourcc!r}, {bits} bit)")
        self.width, self.height = int(width), abs(int(height))
        self._bottom_up = height > 0 and compression == 0
        self._bytes_pp = bits // 8
        self._stride = (self.width * self._bytes_pp + 3) & ~3 if compression == 0 else self.width
        self._lut = None
        self.channels = 1 if bits == 8 else 3
        if bits == 8 and compression == 0 and len(palette) >= 4:
            pal = np.frombuffer(palette[: 4 * (len(palette) // 4)], np.uint8).reshape(-1, 4)[:256, :3]   # B, G, R
            ramp = np.arange(len(pal), dtype=np.uint8)[:, None]
            if not np.array_equal(pal, np.repeat(ramp, 3, axis=1)):
                full = np.zeros((256, 3), np.uint8)
                full[:len(pal)] = pal
                self._lut, self.channels = full, 3
        need = self._stride * self.height
        short = [i for i, f in enumerate(self._frames) if f[1] < need]
        if short:      # dropping them silently would shift every later frame number
            raise ValueError(f"{path}: video chunk {short[0]} holds {self._frames[short[0]][1]} bytes, a frame needs {need}")
        # what the container REPORTS (the stream header's length, cv2's CAP_PROP_FRAME_COUNT) and what it HOLDS: the
        # reference tolerates a report one above the frames it gets and treats anything else as a read error
        # (track_eval.py:170-178); track_bacteria applies that rule to these two numbers
        self.frames_available = len(self._frames)
        self.frame_count = declared[0] or self.frames_available

    def read(self, start, count):
        n = max(0, min(count, self.frames_available - start))
        out = np.empty((n, self.height, self.width) + ((3,) if self.channels == 3 else ()), np.uint8)
        self.read_into(start, n, out)
        return out

    def _chunk(self, i):
        import io
        off, size = self._frames[i]
        self._fh.seek(off)
        return io.BytesIO(self._fh.read(size))

    def _jpeg_first(self, data):
        """(components or None, sampling or None, has DRI) of a frame.  ``sampling`` is the argument of
        ``ysmr_mjpeg_decode_batch`` -- 0 one component, 1 4:4:4, 2 4:2:2, 3 4:2:0 -- if the frame's headers up to SOS pass the
        rules by which that function would not flag it (tests/jpeg_decode_model.py, ``_headers``): SOF0 of this file's size,
        8 bit, the supported sampling factors and component ids, 8-bit DQT, no APP14, no other or second SOF, one scan of all
        components in their order with Ss, Se, Ah / Al = 0, 63, 0, every segment inside the chunk; else None."""
        n, pos = len(data), 2
        components, factors, ids, dri, ok = None, None, None, False, True
        if n < 4 or data[:2] != b"\xff\xd8":
            return None, None, False
        while True:
            if pos >= n or data[pos] != 0xFF:
                return components, None, dri
            while pos < n and data[pos] == 0xFF:                  # fill bytes
                pos += 1
            if pos >= n:
                return components, None, dri
            marker = data[pos]
            pos += 1
            if marker == 0x01 or 0xD0 <= marker <= 0xD8:
                continue
            if marker in (0xD9, 0x00) or pos + 2 > n:
                return components, None, dri
            size = int.from_bytes(data[pos:pos + 2], "big")
            if size < 2 or pos + size > n:
                return components, None, dri
            body = data[pos + 2:pos + size]
            if marker == 0xDB:
                for at in range(0, len(body), 65):
                    if body[at] >> 4 or (body[at] & 15) > 3 or at + 65 > len(body):
                        ok = False                                   # (16-bit table; or damaged)
            elif marker == 0xC0 and components is None and len(body) >= 6 and len(body) == 6 + 3 * body[5]:
                components = body[5]
                ids, factors = [body[6 + 3 * c] for c in range(components)], [body[7 + 3 * c] for c in range(components)]
                if body[0] != 8 or int.from_bytes(body[1:3], "big") != self.height or int.from_bytes(body[3:5], "big") != self.width or \
                        any(body[8 + 3 * c] > 3 for c in range(components)):
                    ok = False
            elif marker == 0xDD:
                dri = len(body) == 2 and int.from_bytes(body, "big") > 0
                ok = ok and len(body) == 2
            elif marker == 0xEE or (0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8)):
                if components is None and 0xC0 <= marker <= 0xCF and marker != 0xCC and len(body) >= 6:
                    components = body[5]                             # (another kind of frame: Pillow's, with this many components)
                ok = False
            elif marker == 0xDA:
                if not ok or components is None or len(body) < 1 or body[0] != components or len(body) != 4 + 2 * components:
                    return components, None, dri
                if [body[1 + 2 * c] for c in range(components)] != ids or any((body[2 + 2 * c] >> 4) > 3 or (body[2 + 2 * c] & 15) > 3
                                                                              for c in range(components)):
                    return components, None, dri
                if tuple(body[1 + 2 * components:]) != (0, 63, 0):
                    return components, None, dri
                if factors == [0x11]:
                    return components, 0, dri
                if ids == [1, 2, 3] and factors[1:] == [0x11, 0x11] and factors[0] in (0x11, 0x21, 0x22):
                    return components, {0x11: 1, 0x21: 2, 0x22: 3}[factors[0]], dri
                return components, None, dri
            pos += size

    def _decode_jpeg(self, blob, dst):
        if self._Image is None:
            raise ValueError(f"{self.path}: Motion-JPEG AVI needs Pillow ({self._no_pillow})")
        with self._Image.open(blob) as im:
            if self.channels == 1:
                dst[...] = np.asarray(im.convert("L"))
            else:
                dst[...] = np.asarray(im.convert("RGB"))[:, :, ::-1]     # BGR, what cv2.VideoCapture delivers

    def read_into(self, start, count, out, pool=None):
        n = max(0, min(count, self.frames_available - start))
        if self._jpeg:
            blobs = [self._chunk(start + i) for i in range(n)]           # file access stays on this thread
            if pool is None:
                for i in range(n):
                    self._decode_jpeg(blobs[i], out[i])
            else:
                for job in [pool.submit(self._decode_jpeg, blobs[i], out[i]) for i in range(n)]:
                    job.result()
            return n
        raw = np.empty((self.height, self._stride), np.uint8)
        used = self.width * self._bytes_pp
        for i in range(n):
            self._fh.seek(self._frames[start + i][0])
            if self._fh.readinto(memoryview(raw).cast("B")) != raw.size:
                raise ValueError(f"{self.path}: frame {start + i} is truncated")
            rows = raw[::-1, :used] if self._bottom_up else raw[:, :used]
            if self._lut is not None:
                out[i] = self._lut[rows]
            elif self.channels == 3:
                out[i] = rows.reshape(self.height, self.width, 3)
            else:
                out[i] = rows
        return n

    # ---- frames as they are in the file, for unpacking on the device (DeviceFrameFeed, ysmr_unpack_dib_batch)
    @property
    def raw_layout(self):
        """None, or what ``ysmr_unpack_dib_batch`` needs to turn the chunk bodies of this file into frames:
        (bytes per stored frame, bytes per pixel, row stride, bottom-up, palette u8 [256, 3] or None)."""
        if self._jpeg:
            return None
        return self._stride * self.height, self._bytes_pp, self._stride, bool(self._bottom_up), self._lut

    def read_raw_into(self, start, count, out, pool=None):
        """Chunk bodies of frames [start, start + count) into ``out[:n]`` (u8 [n, bytes per stored frame], e.g.
        pinned memory): file reads only, no per-pixel work on the host; positional reads (``os.preadv``), spread
        over the threads of ``pool`` if one is given."""
        n = max(0, min(count, self.frames_available - start))
        need = self._stride * self.height
        fd = self._fh.fileno()

        def one(i):
            got, view = 0, memoryview(out[i]).cast("B")[:need]
            while got < need:                                   # (a read may return short of a large request)
                k = os.preadv(fd, [view[got:]], self._frames[start + i][0] + got)
                if k <= 0:
                    raise ValueError(f"{self.path}: frame {start + i} is truncated")
                got += k

        if pool is None or n < 2:
            for i in range(n):
                one(i)
        else:
            for job in [pool.submit(one, i) for i in range(n)]:
                job.result()
        return n

    # ---- Motion-JPEG chunks as they are in the file, for decoding on the device (DeviceFrameFeed, ysmr_mjpeg_decode_batch)
    #: the batch size ``jpeg_layout`` sizes its third number for (a feed asks ``jpeg_layout_for`` with its own)
    jpeg_batch = 248
    def jpeg_layout_for(self, batch, needs_restart=True):
        """None, or what a caller of ``ysmr_mjpeg_decode_batch`` needs to know before it reads this file: (sampling, bytes of
        the largest chunk, most bytes of any ``batch`` consecutive chunks).  None for files that are not Motion-JPEG and for
        those whose first frame is outside the subset the device decodes (``raw_layout`` is None for every JPEG file).
        ``needs_restart``: None also when the first frame has no restart interval (DRI).  One lane decodes a restart interval,
        so a frame without restart markers is one lane's work, and the host path is the faster one for such a file
        (profiles/mjpeg_decode_e2e.log); False gives the layout of every supported file."""
        if not getattr(self, "_jpeg", False) or self._jpeg_sampling is None or (needs_restart and not self._jpeg_dri):
            return None
        sizes = np.array([f[1] for f in self._frames], np.int64)
        total = np.concatenate([[0], np.cumsum(sizes)])
        k = max(1, min(int(batch), len(sizes)))
        return self._jpeg_sampling, int(sizes.max()), int((total[k:] - total[:-k]).max())

    @property
    def jpeg_layout(self):
        return self.jpeg_layout_for(self.jpeg_batch)

    def read_jpeg_into(self, start, count, out, offsets, pool=None):
        """Chunk bodies of frames [start, start + count) back to back into ``out`` (u8 [bytes], e.g. pinned memory; the
        RIFF pad byte of an odd-sized chunk is not part of it) and where each begins into ``offsets[:n + 1]`` (int64): file
        reads only (``os.preadv``, spread over the threads of ``pool`` if one is given), nothing is parsed."""
        n = max(0, min(count, self.frames_available - start))
        fd = self._fh.fileno()
        at = 0
        for i in range(n):
            offsets[i] = at
            at += self._frames[start + i][1]
        offsets[n] = at
        if at > out.size:
            raise ValueError(f"{self.path}: frames {start} .. {start + n - 1} hold {at} bytes, the buffer {out.size}")
        flat = memoryview(out).cast("B")

        def one(i):
            where, need = self._frames[start + i]
            got, view = 0, flat[int(offsets[i]):int(offsets[i]) + need]
            while got < need:
                k = os.preadv(fd, [view[got:]], where + got)
                if k <= 0:
                    raise ValueError(f"{self.path}: frame {start + i} is truncated")
                got += k

        if pool is None or n < 2:
            for i in range(n):
                one(i)
        else:
            for job in [pool.submit(one, i) for i in range(n)]:
                job.result()
        return n

    def close(self):
        self._fh.close()


class TiffVideo:
    """Multi-page TIFF stack (what ImageJ / Fiji, Micro-Manager, Bio-Formats and camera software write) without OpenCV, and
    without Pillow where it can be: classic TIFF of either byte order, one page per frame.

    Served natively -- the host path reads uncompressed strips itself, ``DeviceFrameFeed`` uploads the stored strips and
    ``ysmr_tiff_decode_batch`` decodes them -- are pages of 8 bits per sample, photometric 0 (WhiteIsZero, delivered inverted as
    Pillow delivers it), 1 (BlackIsZero) or 2 (RGB, delivered B, G, R), one sample per pixel or three chunky ones, compression 1
    (none), 5 (LZW, MSB first) or 32773 (PackBits), predictor 1 or 2, in strips, every page like the first.  Anything else --
    deflate, JPEG, tiles, palettes, 16 bit, planar RGB, extra samples, old-style LZW, a page unlike the first -- is decoded by
    Pillow page by page, with whatever Pillow raises; without Pillow it is a ValueError naming the tag.  BigTIFF is refused.
    ImageJ's convention for stacks above 4 GB (ONE directory, ``images=N`` in the description, the planes behind one another)
    is not followed: such a file reads as the one page its directory describes.

    TIFF has no frame rate: ``fps`` is ``default_fps`` (tracking.ini's 'frames per second')."""

    _SIZES = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
    _LETTER = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i", 13: "I"}
    _NAMES = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 262: "PhotometricInterpretation",
              266: "FillOrder", 273: "StripOffsets", 277: "SamplesPerPixel", 278: "RowsPerStrip", 279: "StripByteCounts",
              284: "PlanarConfiguration", 317: "Predictor", 322: "TileWidth", 338: "ExtraSamples"}

    def __init__(self, path, default_fps=30.0):
        import logging
        import threading
        self.path = path
        self._fh = open(path, "rb")
        try:
            self._parse(path)
        except BaseException:
            self._fh.close()
            raise
        self.fps = float(default_fps)
        self._local, self._opened = threading.local(), []
        logging.getLogger("ysmr").info("%s: a TIFF stack carries no frame rate; using 'frames per second' = %s", path, self.fps)

    # ---- the directories
    def _parse(self, path):
        import struct
        fh = self._fh
        size = os.path.getsize(path)
        head = fh.read(8)
        if len(head) < 8 or head[:2] not in (b"II", b"MM"):
            raise ValueError(f"{path}: not a TIFF file")
        e = self._endian = "<" if head[:2] == b"II" else ">"
        version, at = struct.unpack(e + "HI", head[2:])
        if version == 43:
            raise ValueError(f"{path}: BigTIFF (version 43) is not read; save the stack as classic TIFF")
        if version != 42:
            raise ValueError(f"{path}: not a TIFF file (version {version})")
        wanted = set(self._NAMES)
        self._pages, seen = [], set()
        while at:
            if at in seen or at + 2 > size:
                raise ValueError(f"{path}: damaged directory chain at offset {at}")
            seen.add(at)
            fh.seek(at)
            (count,) = struct.unpack(e + "H", fh.read(2))
            raw = fh.read(12 * count + 4)
            if len(raw) < 12 * count + 4:
                raise ValueError(f"{path}: directory at offset {at} is truncated")
            tags = {}
            for k in range(count):
                tag, kind, n = struct.unpack(e + "HHI", raw[12 * k:12 * k + 8])
                if tag not in wanted:
                    continue
                letter, width = self._LETTER.get(kind), self._SIZES.get(kind, 0)
                if letter is None:
                    raise ValueError(f"{path}: tag {tag} ({self._NAMES[tag]}) has type {kind}")
                if n * width <= 4:
                    data = raw[12 * k + 8:12 * k + 8 + n * width]
                else:
                    (where,) = struct.unpack(e + "I", raw[12 * k + 8:12 * k + 12])
                    fh.seek(where)
                    data = fh.read(n * width)
                    if len(data) < n * width:
                        raise ValueError(f"{path}: tag {tag} ({self._NAMES[tag]}) points outside the file")
                tags[tag] = np.frombuffer(data, np.dtype(e + {"B": "u1", "H": "u2", "I": "u4", "b": "i1", "h": "i2", "i": "i4"}[letter]),
                                          n).astype(np.int64)
            self._pages.append(tags)
            (at,) = struct.unpack(e + "I", raw[12 * count:])
        if not self._pages:
            raise ValueError(f"{path}: no pages")
        first = self._pages[0]
        if 256 not in first or 257 not in first:
            raise ValueError(f"{path}: the first directory has no ImageWidth / ImageLength")
        self.width, self.height = int(first[256][0]), int(first[257][0])
        self.frame_count = self.frames_available = len(self._pages)
        try:
            from PIL import Image
            self._Image, self._no_pillow = Image, None
        except ImportError as exc:
            self._Image, self._no_pillow = None, str(exc)
        self._why = [self._outside(k) for k in range(len(self._pages))]      # None: the page is in the native subset
        if self._why[0] is None:
            self.channels = int(self._tag(first, 277, 1))
            self._compression, self._predictor = int(self._tag(first, 259, 1)), int(self._tag(first, 317, 1))
            self._photometric = int(self._tag(first, 262, 1))
            self._rows_per_strip = min(self.height, int(self._tag(first, 278, self.height)))
            self._strips_per_frame = -(-self.height // self._rows_per_strip)
        elif self._Image is None:
            raise ValueError(f"{path}: {self._why[0]}; such a file needs Pillow ({self._no_pillow})")
        else:
            with self._Image.open(path) as im:
                self.channels = 1 if im.mode in ("1", "L", "I", "F") or im.mode.startswith("I;16") else 3

    @staticmethod
    def _tag(tags, tag, default):
        return tags[tag][0] if tag in tags and len(tags[tag]) else default

    _SAME = (256, 257, 258, 259, 262, 277, 278, 284, 317)

    def _outside(self, k):
        """None, or why page k is not in the native subset: '<tag name> <tag> = <value>'."""
        tags, first = self._pages[k], self._pages[0]

        def says(tag, value):
            return "page {}: {} ({}) = {}".format(k, self._NAMES[tag], tag, value)

        samples = int(self._tag(tags, 277, 1))
        bits = [int(b) for b in tags.get(258, [1])]
        if any(b != 8 for b in bits):
            return says(258, bits if len(bits) > 1 else bits[0])
        if samples not in (1, 3) or 338 in tags:
            return says(338, list(tags[338])) if 338 in tags else says(277, samples)
        photometric = int(self._tag(tags, 262, -1))
        if photometric not in ((0, 1) if samples == 1 else (2,)):
            return says(262, photometric)
        if int(self._tag(tags, 259, 1)) not in (1, 5, 32773):
            return says(259, int(self._tag(tags, 259, 1)))
        if int(self._tag(tags, 317, 1)) not in (1, 2):
            return says(317, int(self._tag(tags, 317, 1)))
        if samples == 3 and int(self._tag(tags, 284, 1)) != 1:
            return says(284, int(self._tag(tags, 284, 1)))
        if int(self._tag(tags, 266, 1)) != 1:
            return says(266, int(self._tag(tags, 266, 1)))
        if 322 in tags:
            return says(322, int(tags[322][0]))
        if 273 not in tags or 279 not in tags:
            return "page {}: no StripOffsets (273) / StripByteCounts (279)".format(k)
        height, width = int(self._tag(tags, 257, 0)), int(self._tag(tags, 256, 0))
        if height <= 0 or width <= 0:
            return says(257, height)
        rows = min(height, int(self._tag(tags, 278, height)))
        if rows <= 0:
            return says(278, rows)
        strips = -(-height // rows)
        if len(tags[273]) != strips or len(tags[279]) != strips:
            return says(273, "{} offsets, {} rows in strips of {}".format(len(tags[273]), height, rows))
        for tag in self._SAME:
            if k and int(self._tag(tags, tag, 1 if tag != 278 else height)) != int(self._tag(first, tag, 1 if tag != 278 else height)):
                return says(tag, "{}, the first page has {}".format(int(self._tag(tags, tag, 1)), int(self._tag(first, tag, 1))))
        if int(self._tag(tags, 259, 1)) == 5:          # libtiff's test for the old LSB-first LZW
            for where, size in zip(tags[273], tags[279]):
                self._fh.seek(int(where))
                start = self._fh.read(2)
                if size >= 2 and len(start) == 2 and start[0] == 0 and start[1] & 1:
                    return says(259, "5 in its old LSB-first form")
                break                                     # (the first strip tells; a later one is the device's to flag)
        return None

    @property
    def native(self):
        """Every page is in the subset this reader and the device serve without Pillow."""
        return all(w is None for w in self._why)

    def strips_of(self, k):
        """(offsets, byte counts) of page k, int64 arrays."""
        return self._pages[k][273], self._pages[k][279]

    # ---- the host path
    def read(self, start, count):
        n = max(0, min(count, self.frames_available - start))
        out = np.empty((n, self.height, self.width) + ((3,) if self.channels == 3 else ()), np.uint8)
        self.read_into(start, n, out)
        return out

    def _pillow_page(self, k, dst):
        if self._Image is None:
            raise ValueError(f"{self.path}: {self._why[k] or 'a compressed page'}; the host path needs Pillow ({self._no_pillow})")
        im = getattr(self._local, "im", None)
        if im is None:
            im = self._local.im = self._Image.open(self.path)        # (one per reader thread: a seek walks the directories)
            self._opened.append(im)
        im.seek(k)
        if self.channels == 1:
            dst[...] = np.asarray(im.convert("L"))
        else:
            dst[...] = np.asarray(im.convert("RGB"))[:, :, ::-1]         # B, G, R: what cv2.VideoCapture delivers

    def _decode_page(self, k, dst):
        """Page k into ``dst`` on the host: uncompressed strips of the native subset by this reader, the rest by Pillow."""
        if self._why[k] is not None or self._compression != 1:
            return self._pillow_page(k, dst)
        offsets, counts = self.strips_of(k)
        row_bytes = self.width * self.channels
        plain = self._predictor == 1 and self._photometric == 1 and dst.flags["C_CONTIGUOUS"]
        raw = dst.reshape(-1) if plain else np.empty(self.height * row_bytes, np.uint8)
        fd = self._fh.fileno()
        for s in range(len(offsets)):
            lo = s * self._rows_per_strip * row_bytes
            need = min(self._rows_per_strip, self.height - s * self._rows_per_strip) * row_bytes
            if counts[s] < need:
                raise ValueError(f"{self.path}: page {k}, strip {s} holds {counts[s]} bytes, its rows need {need}")
            view, got = memoryview(raw[lo:lo + need]), 0
            while got < need:
                n = os.preadv(fd, [view[got:]], int(offsets[s]) + got)
                if n <= 0:
                    raise ValueError(f"{self.path}: page {k} is truncated")
                got += n
        if not plain:
            a = raw.reshape(self.height, self.width, self.channels)
            if self._predictor == 2:
                a = np.cumsum(a, axis=1, dtype=np.uint32).astype(np.uint8)
            if self._photometric == 0:
                a = ~a
            dst[...] = a[:, :, ::-1] if self.channels == 3 else a[:, :, 0]

    def read_into(self, start, count, out, pool=None):
        n = max(0, min(count, self.frames_available - start))
        if pool is None or n < 2:
            for i in range(n):
                self._decode_page(start + i, out[i])
        else:
            for job in [pool.submit(self._decode_page, start + i, out[i]) for i in range(n)]:
                job.result()
        return n

    # ---- strips as they are in the file, for decoding on the device (DeviceFrameFeed, ysmr_tiff_decode_batch)
    def tiff_layout_for(self, batch):
        """None, or what a caller of ``ysmr_tiff_decode_batch`` needs to know before it reads this file: (compression, predictor,
        photometric, rows per strip, strips per frame, most body bytes of any ``batch`` consecutive pages).  None where a page
        is outside the native subset, and where the device entry refuses the sizes.  (A page of ONE strip is one wave's serial
        work on the device, and still faster there than on the host: profiles/tiff_decode_e2e.log.)"""
        if not self.native:
            return None
        sizes = np.array([int(p[279].sum()) for p in self._pages], np.int64)
        total = np.concatenate([[0], np.cumsum(sizes)])
        k = max(1, min(int(batch), len(sizes)))
        most = int((total[k:] - total[:-k]).max())
        from . import _lib
        if _lib.lib().ysmr_tiff_decode_workspace_bytes(int(batch), self.height, self.width, self.channels, self._compression,
                                                       self._predictor, self._photometric, self._rows_per_strip, most) == 0:
            return None
        return self._compression, self._predictor, self._photometric, self._rows_per_strip, self._strips_per_frame, most

    def read_tiff_into(self, start, count, out, table, pool=None):
        """Strip bodies of pages [start, start + count) back to back into ``out`` (u8 [bytes], e.g. pinned memory) and the
        strip table into ``table[:n * strips per frame]`` (int32 [.., 5]: frame of the batch, first row, rows, offset in
        ``out``, bytes): file reads only (``os.preadv``, strips that follow one another in the file in one read, spread over
        the threads of ``pool`` if one is given), nothing is decoded.  Returns (pages, bytes used)."""
        n = max(0, min(count, self.frames_available - start))
        fd, spf, rps = self._fh.fileno(), self._strips_per_frame, self._rows_per_strip
        at, reads = 0, []
        for i in range(n):
            offsets, counts = self.strips_of(start + i)
            rows = table[i * spf:(i + 1) * spf]
            rows[:, 0] = i
            rows[:, 1] = np.arange(spf) * rps
            rows[:, 2] = np.minimum(rps, self.height - rows[:, 1])
            rows[:, 3] = at + np.concatenate([[0], np.cumsum(counts[:-1])])
            rows[:, 4] = counts
            ends = offsets + counts
            cuts = np.flatnonzero(offsets[1:] != ends[:-1]) + 1          # where a strip does not follow its predecessor
            for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [spf]])):
                reads.append((int(offsets[lo]), int(rows[lo, 3]), int(counts[lo:hi].sum()), start + i))
            at += int(counts.sum())
        if at > out.size:
            raise ValueError(f"{self.path}: pages {start} .. {start + n - 1} hold {at} bytes, the buffer {out.size}")
        flat = memoryview(out).cast("B")

        def one(job):
            where, to, need, page = job
            got, view = 0, flat[to:to + need]
            while got < need:
                k = os.preadv(fd, [view[got:]], where + got)
                if k <= 0:
                    raise ValueError(f"{self.path}: page {page} is truncated")
                got += k

        if pool is None or len(reads) < 2:
            for job in reads:
                one(job)
        else:
            for job in [pool.submit(one, job) for job in reads]:
                job.result()
        return n, at

    def close(self):
        self._fh.close()
        while self._opened:
            self._opened.pop().close()


class Cv2Video:
    """Fallback for compressed containers when OpenCV is installed (decode stays on the host)."""

    def __init__(self, path, default_fps=30.0):
        import cv2  # noqa: F401  (optional dependency)
        self._cv2 = cv2
        self._cap = cv2.VideoCapture(path)
        self.frame_count = int(self._cap.get(cv2.CAP_PROP_FRAME_COUNT))   # what the container reports ...
        self.frames_available = 1 << 62                                    # ... read() tells where it really ends
        self.fps = float(self._cap.get(cv2.CAP_PROP_FPS) or default_fps)
        self.height, self.width = int(self._cap.get(4)), int(self._cap.get(3))
        self.channels = 3
        self._next = 0

    def read(self, start, count):
        if start != self._next:
            self._cap.set(self._cv2.CAP_PROP_POS_FRAMES, start)
        frames = []
        for _ in range(count):
            ok, frame = self._cap.read()
            if not ok:
                break
            frames.append(frame)
        self._next = start + len(frames)
        if not frames:
            return np.empty((0, self.height, self.width, 3), np.uint8)
        return np.stack(frames)

    def close(self):
        self._cap.release()


_NODE_CPUS = {}      # GPU index -> CPUs of its NUMA node (sysfs; asked once per process)


def cpus_near_gpu(device):
    """The CPUs of the NUMA node the GPU hangs off that this thread may use (None: unknown, or fewer than four)."""
    try:
        import torch
        from . import dist
        index = torch.device(device).index or 0
        if index not in _NODE_CPUS:
            _NODE_CPUS[index] = dist.local_cpus(dist.pci_bus_id(index))
        cpus = _NODE_CPUS[index]
        if not cpus:
            return None
        cpus = cpus & os.sched_getaffinity(0)
        return cpus if len(cpus) >= 4 else None
    except (AttributeError, OSError, ValueError):
        return None


class _ThreadOn:
    """``with _ThreadOn(cpus):`` -- the calling THREAD runs on ``cpus`` inside the block (Linux: sched_setaffinity(0) is the
    calling thread's mask, and the threads it starts inherit it), and on what it was allowed before afterwards."""

    def __init__(self, cpus):
        self.cpus, self.before = cpus, None

    def __enter__(self):
        if self.cpus:
            try:
                self.before = os.sched_getaffinity(0)
                os.sched_setaffinity(0, self.cpus)
            except (AttributeError, OSError):
                self.before = None
        return self

    def __exit__(self, *exc):
        if self.before is not None:
            try:
                os.sched_setaffinity(0, self.before)
            except OSError:
                pass
        return False


class DeviceFrameFeed:
    """Batches of a video as device tensors, read and uploaded ahead of their use.

    A producer thread copies batch i into one of ``depth`` pinned staging buffers (split over
    ``readers`` threads) and uploads it on its own HIP stream into one of ``depth`` device buffers,
    while the consumer works on earlier batches.  Iterating yields ``(frames_dev, first_frame, count,
    slot)``; the consumer's stream already waits for the upload.  When the kernels that read
    ``frames_dev`` have been issued, the consumer calls ``release(slot, event)`` with an event recorded
    behind them: the slot's device buffer is overwritten only after that event.

    ``near_gpu``: the staging buffers are allocated, and the producer and its readers run, on the CPUs of the GPU's own NUMA node
    (the caller's threads are left where they are).  On a two-socket host the copy into pinned memory and the DMA out of it
    otherwise cross the sockets' link half of the time: reads 50-60 GB/s and uploads 35-45 while both run, against 85-90 and
    56 (`scripts/feed_copy_timeline.py`).

    ``decode_on_device`` (the settings key 'hip decode mjpeg'): True -- a Motion-JPEG AVI whose ``jpeg_layout`` is not None (a
    supported first frame WITH a restart interval) -- or "always" -- also one without restart markers -- is uploaded as chunk
    bodies and decoded on the copy stream: by ``ysmr_mjpeg_decode_batch``, a lane per restart interval, or under "always" by
    ``ysmr_mjpeg_decode_batch_sync``, which decodes a frame without restart markers with a lane per 64 bytes of its entropy data
    (and one with them as the other call does); the per-frame status comes back once per batch, and a frame it flags
    (outside the supported subset, or damaged) is decoded again by the host path and copied into its place -- with whatever
    that path raises.  False: every frame takes the host path.

    ``decode_tiff`` (the settings key 'hip decode tiff'): True -- a TIFF stack whose ``tiff_layout_for`` is not None is uploaded as
    [strip table][strip bodies as stored] and decoded on the copy stream by ``ysmr_tiff_decode_batch``, with the same handling
    of flagged frames.  False: the host path."""

    def __init__(self, video, batch, device, depth=3, readers=16, pieces=4, near_gpu=True, decode_on_device=True, decode_tiff=True):
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor

        import torch
        self.video, self.B, self.device, self.depth = video, int(batch), torch.device(device), int(depth)
        self.pieces = max(1, int(pieces))
        shape = (self.B, video.height, video.width) + ((3,) if video.channels == 3 else ())
        # uncompressed AVI: the stored frames (bottom-up, padded rows, palette indices) go to the device as they are
        # and are unpacked there; every other source delivers finished frames
        self._raw = getattr(video, "raw_layout", None)
        # Motion-JPEG AVI: the chunk bodies go to the device as they are and are decoded there
        if decode_on_device not in (True, False, "always"):
            raise ValueError("decode_on_device must be True, False or 'always', got {!r}".format(decode_on_device))
        self._decode_on_device = decode_on_device
        self._jpeg = video.jpeg_layout_for(self.B, needs_restart=decode_on_device != "always") \
            if decode_on_device and hasattr(video, "jpeg_layout_for") else None
        # TIFF stack: the strips go to the device as they are stored and are decoded there
        self._tiff = video.tiff_layout_for(self.B) if decode_tiff and hasattr(video, "tiff_layout_for") else None
        self._stored = self._jpeg is not None or self._tiff is not None
        self._cpus = cpus_near_gpu(self.device) if near_gpu else None
        with _ThreadOn(self._cpus):      # (pinned pages are the calling thread's node's)
            self._allocate(shape)
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._uploaded = [None] * self.depth     # event: H2D copy out of pinned[slot] finished
        self._released = [None] * self.depth     # event posted by the consumer (or True: never used / free)
        self._cv = threading.Condition()
        for k in range(self.depth):
            self._released[k] = True
        self._q = queue.Queue(maxsize=self.depth)
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(readers))) if readers > 1 else None
        self._stop = False
        self._thread = threading.Thread(target=self._produce, name="ysmr-frame-feed", daemon=True)
        self._thread.start()

    def _allocate(self, shape):
        import torch
        if self._stored:
            from . import _lib
            # [head: where the pieces lie] [the bytes as stored]: one copy per batch, of the bytes used
            if self._jpeg is not None:
                sampling, _, batch_bytes = self._jpeg
                self._stored_head = 8 * (self.B + 1)                          # offsets int64 [B + 1], then the chunk bodies
            else:
                batch_bytes = self._tiff[5]
                self._stored_head = (20 * self.B * self._tiff[4] + 255) // 256 * 256   # strips int32 [B * strips per frame][5], then their bodies
            size = self._stored_head + batch_bytes
            self._pinned = [torch.empty(size, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
            self._stored_dev = [torch.empty(size, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
            self._status_dev = [torch.empty(self.B, dtype=torch.int32, device=self.device) for _ in range(self.depth)]
            self._status = [torch.empty(self.B, dtype=torch.int32, pin_memory=True) for _ in range(self.depth)]
            self._frame_host = torch.empty(shape[1:], dtype=torch.uint8, pin_memory=True)       # for a frame the host decodes
        if self._tiff is not None:
            compression, predictor, photometric, rows_per_strip, _, batch_bytes = self._tiff
            ws = _lib.lib().ysmr_tiff_decode_workspace_bytes(self.B, shape[1], shape[2], self.video.channels, compression, predictor,
                                                             photometric, rows_per_strip, batch_bytes)
            if ws == 0:
                raise ValueError("ysmr_tiff_decode_workspace_bytes refuses {} frames of {} x {}".format(self.B, shape[2], shape[1]))
            self._stored_ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        elif self._jpeg is not None:
            # 'always': the entry that also decodes a frame without restart markers with many lanes; it sizes its workspace
            # by the file's largest chunk
            self._jpeg_sync = self._decode_on_device == "always"
            if self._jpeg_sync:
                ws = _lib.lib().ysmr_mjpeg_decode_sync_workspace_bytes(self.B, shape[1], shape[2], self.video.channels, sampling,
                                                                       self._jpeg[1])
            else:
                ws = _lib.lib().ysmr_mjpeg_decode_workspace_bytes(self.B, shape[1], shape[2], self.video.channels, sampling)
            if ws == 0:
                raise ValueError("ysmr_mjpeg_decode_{}workspace_bytes refuses {} frames of {} x {} (largest chunk {} bytes)".format(
                    "sync_" if self._jpeg_sync else "", self.B, shape[2], shape[1], self._jpeg[1]))
            self._stored_ws = torch.empty(ws, dtype=torch.uint8, device=self.device)           # (the slots' decodes are serial)
        elif self._raw is not None:
            raw_bytes, _, _, _, palette = self._raw
            self._pinned = [torch.empty((self.B, raw_bytes), dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
            self._raw_dev = [torch.empty((self.B, raw_bytes), dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
            self._palette = None if palette is None else torch.from_numpy(np.ascontiguousarray(palette)).to(self.device)
        else:
            self._pinned = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self._dev = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]

    def _produce(self):
        import torch
        try:
            torch.cuda.set_device(self.device)
            if self._cpus:
                try:
                    os.sched_setaffinity(0, self._cpus)      # this thread, and the readers it starts
                except OSError:
                    pass
            i = 0
            # (every frame the source HOLDS, which need not be the number it reports: track_bacteria applies the
            # reference's rule to the difference)
            for f0 in range(0, getattr(self.video, "frames_available", self.video.frame_count), self.B):
                slot = i % self.depth
                with self._cv:
                    busy = self._released[slot] is None
                if busy:
                    self._finish_stored()      # (the consumer frees this slot only after it has been given what is pending)
                with self._cv:
                    while self._released[slot] is None and not self._stop:
                        self._cv.wait(0.05)
                    if self._stop:
                        return
                    released, self._released[slot] = self._released[slot], None
                if self._uploaded[slot] is not None:
                    self._uploaded[slot].synchronize()          # staging buffer free again
                host = self._pinned[slot].numpy()
                if self._stored:
                    n = self._produce_stored(f0, slot, released, host)
                    if n == 0:
                        break
                    i += 1
                    continue
                # A batch is read and uploaded in `pieces` parts: the upload of a part starts when the part has been read, not
                # when the batch has (the first batch of a 1228 x 922 file is 280 MB: 5 ms of reading before the first byte
                # crossed the bus, 4 of the 73 ms a 1920-frame file takes)
                step = max(1, -(-self.B // self.pieces))
                n = 0
                for c0 in range(0, self.B, step):
                    want = min(step, self.B - c0)
                    if self._raw is not None:
                        got = self.video.read_raw_into(f0 + c0, want, host[c0:c0 + want], self._pool)
                    elif hasattr(self.video, "read_into"):
                        got = self.video.read_into(f0 + c0, want, host[c0:c0 + want], self._pool)
                    else:
                        part = self.video.read(f0 + c0, want)
                        got = part.shape[0]
                        host[c0:c0 + got] = part
                    if got:
                        with torch.cuda.stream(self._copy_stream):
                            if released is not True:
                                self._copy_stream.wait_event(released)  # the kernels that read this device buffer are done
                                released = True
                            dst = self._raw_dev[slot] if self._raw is not None else self._dev[slot]
                            dst[c0:c0 + got].copy_(self._pinned[slot][c0:c0 + got], non_blocking=True)
                    n += got
                    if got < want:
                        break
                if n == 0:
                    break
                with torch.cuda.stream(self._copy_stream):
                    if self._raw is not None:
                        from . import _lib
                        raw_bytes, bpp, stride, bottom_up, _ = self._raw
                        _lib.check(_lib.lib().ysmr_unpack_dib_batch(
                            self._copy_stream.cuda_stream, self._raw_dev[slot].data_ptr(), n, raw_bytes, self.video.height,
                            self.video.width, bpp, stride, int(bottom_up),
                            None if self._palette is None else self._palette.data_ptr(), self._dev[slot].data_ptr()),
                            "ysmr_unpack_dib_batch")
                    ev = torch.cuda.Event()
                    ev.record(self._copy_stream)
                self._uploaded[slot] = ev
                self._q.put((slot, f0, n, ev))
                i += 1
            self._finish_stored()
            self._q.put(None)
        except BaseException as exc:   # hand the failure to the consumer
            self._q.put(exc)

    _stored_pending = None

    def _produce_stored(self, f0, slot, released, host):
        """Batch ``f0`` as it is stored (Motion-JPEG chunk bodies, or TIFF strips): read, upload, decode on the copy stream.  The
        batch is handed on when its status has come back, which is waited for only after the NEXT batch has been read and
        issued (``_finish_stored``)."""
        import torch
        video, head = self.video, self._stored_head
        if self._jpeg is not None:
            offsets = host[:head].view(np.int64)
            n = video.read_jpeg_into(f0, self.B, host[head:], offsets, self._pool)
            used = head + int(offsets[n])
        else:
            table = host[:20 * self.B * self._tiff[4]].view(np.int32).reshape(-1, 5)
            n, body_bytes = video.read_tiff_into(f0, self.B, host[head:], table, self._pool)
            used = head + body_bytes
        if n == 0:
            return 0
        with torch.cuda.stream(self._copy_stream):
            if released is not True:
                self._copy_stream.wait_event(released)          # the kernels that read this device buffer are done
            self._stored_dev[slot][:used].copy_(self._pinned[slot][:used], non_blocking=True)
            self._decode_stored(slot, n)
            self._status[slot][:n].copy_(self._status_dev[slot][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        self._uploaded[slot] = ev
        self._finish_stored()
        self._stored_pending = (slot, f0, n, ev)
        return n

    def _decode_stored(self, slot, n):
        """The decode of the ``n`` frames uploaded into ``slot``, issued on the copy stream."""
        from . import _lib
        video, head, L = self.video, self._stored_head, _lib.lib()
        stream, stored = self._copy_stream.cuda_stream, self._stored_dev[slot].data_ptr()
        ws, frames, status = self._stored_ws, self._dev[slot].data_ptr(), self._status_dev[slot].data_ptr()
        if self._tiff is not None:
            compression, predictor, photometric, _, strips_per_frame, _ = self._tiff
            _lib.check(L.ysmr_tiff_decode_batch(stream, stored + head, stored, n * strips_per_frame, n, video.height, video.width,
                                                video.channels, compression, predictor, photometric, ws.data_ptr(), ws.numel(), frames,
                                                status), "ysmr_tiff_decode_batch")
        elif self._jpeg_sync:
            _lib.check(L.ysmr_mjpeg_decode_batch_sync(stream, stored + head, stored, n, video.height, video.width, video.channels,
                                                      self._jpeg[0], self._jpeg[1], ws.data_ptr(), ws.numel(), frames, status),
                       "ysmr_mjpeg_decode_batch_sync")
        else:
            _lib.check(L.ysmr_mjpeg_decode_batch(stream, stored + head, stored, n, video.height, video.width, video.channels,
                                                 self._jpeg[0], ws.data_ptr(), ws.numel(), frames, status), "ysmr_mjpeg_decode_batch")

    def _host_frame(self, k, dst):
        """Frame ``k`` by the video's host path."""
        if self._tiff is not None:
            self.video._decode_page(k, dst)
        else:
            self.video._decode_jpeg(self.video._chunk(k), dst)

    def _finish_stored(self):
        """Hand the pending batch of stored bytes to the consumer: its status is here once its event has passed; the frames the
        device flagged are decoded by the host path (which raises what it raises today) and copied into their places."""
        import torch
        if self._stored_pending is None:
            return
        (slot, f0, n, ev), self._stored_pending = self._stored_pending, None
        ev.synchronize()
        flagged = np.flatnonzero(self._status[slot][:n].numpy())
        if len(flagged):
            with torch.cuda.stream(self._copy_stream):
                for k in flagged:
                    self._host_frame(f0 + int(k), self._frame_host.numpy())
                    self._dev[slot][int(k)].copy_(self._frame_host, non_blocking=True)
                    self._copy_stream.synchronize()             # (the one staging frame is free again)
                ev = torch.cuda.Event()
                ev.record(self._copy_stream)
            self._uploaded[slot] = ev
        self._q.put((slot, f0, n, ev))

    def __iter__(self):
        import torch
        while True:
            item = self._q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            slot, f0, n, ev = item
            torch.cuda.current_stream(self.device).wait_event(ev)
            yield self._dev[slot][:n], f0, n, slot

    def release(self, slot, event):
        with self._cv:
            self._released[slot] = event
            self._cv.notify_all()

    def close(self):
        self._stop = True
        with self._cv:
            self._cv.notify_all()
        try:
            while True:                # unblock a producer waiting on a full queue
                self._q.get_nowait()
        except Exception:
            pass
        self._thread.join(timeout=5.0)
        if self._pool is not None:
            self._pool.shutdown(wait=False)


def decode_mjpeg_setting(settings):
    """The ``decode_on_device`` argument of ``DeviceFrameFeed`` from the optional settings key 'hip decode mjpeg': true
    (default: Motion-JPEG files with restart markers are decoded on the device), false (every frame by the host path) or
    'always' (files without restart markers too, by ``ysmr_mjpeg_decode_batch_sync``: what cameras, ffmpeg, OpenCV and Pillow
    write; profiles/mjpeg_decode_sync_e2e.log has the rates)."""
    value = settings.get("hip decode mjpeg", True)
    if isinstance(value, str):
        word = value.strip().lower()
        if word == "always":
            return "always"
        return word not in ("false", "0", "no", "off", "")
    return bool(value)


#: what 'hip decode tiff' is without the key: on one MI355X the device path's whole range lay above the host path's on the LZW file
#: with libtiff's default strips (6.3 - 6.5 k frames/s against 409 - 460, profiles/tiff_decode_e2e.log)
DECODE_TIFF_DEFAULT = True


def decode_tiff_setting(settings):
    """The ``decode_tiff`` argument of ``DeviceFrameFeed`` from the optional settings key 'hip decode tiff': true -- a TIFF stack
    that ``TiffVideo.tiff_layout_for`` serves is uploaded as stored strips and decoded on the device -- or false -- every frame
    by the host path (uncompressed strips read directly, compressed ones by Pillow on the reader threads).  Without the key:
    ``DECODE_TIFF_DEFAULT``."""
    value = settings.get("hip decode tiff", DECODE_TIFF_DEFAULT)
    if isinstance(value, str):
        return value.strip().lower() not in ("false", "0", "no", "off", "")
    return bool(value)


def open_video(path, default_fps=30.0):
    ext = os.path.splitext(path)[1].lower()
    if ext in (".tif", ".tiff"):
        return TiffVideo(path, default_fps)
    if ext == ".npy":
        return NpyVideo(path, default_fps)
    if ext == ".y4m":
        return Y4mVideo(path, default_fps)
    if ext == ".avi":
        try:
            return AviVideo(path, default_fps)
        except ValueError:
            pass                                   # compressed: OpenCV's business
    try:
        return Cv2Video(path, default_fps)
    except ImportError as exc:
        raise OSError(f"{path}: only .npy and .y4m can be read without OpenCV ({exc})") from exc
