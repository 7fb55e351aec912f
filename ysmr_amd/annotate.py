"""``annotate_video`` -- the annotated output video on the device (ysmr/track_eval.py:1321-1472).

Upstream reads the video again, paints every track's id and centroid into each frame (``cv2.putText``, ``cv2.circle``)
and hands the frames to ``cv2.VideoWriter``.  Here the frames come through ``DeviceFrameFeed``, ``ysmr_annotate_batch``
(``csrc/annotate.hip``) paints the marks and lays the frames out as stored 24-bit DIB frames, and then either

* (uncompressed, the default) a stream of its own copies them into one of two pinned buffers, and a writer thread appends
  those to an uncompressed AVI (``AviWriter``), or
* (Motion-JPEG: 'save video file extension' ``.avi`` with 'save video fourcc codec' ``MJPG`` / ``JPEG``)
  ``ysmr_mjpeg_encode_batch`` (``csrc/mjpeg.hip``) turns them into finished ``00dc`` chunks, one baseline JPEG each, on the
  device; the copy stream brings over their offsets and then only the bytes those name, and the writer thread appends
  them to a Motion-JPEG AVI (``MjpegAviWriter``).

Either way the host moves bytes and touches no pixel.  The way from the painted device buffer to the file -- two slots, the
copy stream, the pinned buffers, the writer thread, the encode call -- is ``DibOutput``; the detection view and the
threshold view of ``track_bacteria`` ('hip save detection video', 'hip save threshold video': ``track_eval._DetectionView``,
``_ThresholdView``) leave through it as well.

Departures from upstream, all deliberate:

* the file is always an ``.avi``, uncompressed 24-bit or Motion-JPEG (no encoder is a dependency of this package: the
  JPEG encoder is the package's own kernels); settings that ask for another container or codec are answered with one
  warning that names what is written;
* Motion-JPEG is, unless asked otherwise, 4:4:4 with the typical Huffman tables of T.81 Annex K at the quality of the
  optional settings key 'hip video jpeg quality' (1 .. 100, default 90), one restart interval per MCU row
  (``output_format``).  Upstream's ``cv2.VideoWriter`` writes 4:2:0: 'hip video jpeg subsampling' = '4:2:0' (or '4:2:2')
  does so too, and 'hip video jpeg huffman' = 'optimised' gives every frame Huffman tables built from its own symbols
  (``jpeg_mode``; ``ysmr_mjpeg_encode_batch``);
* the digits are a 5 x 7 bitmap font, not OpenCV's Hershey strokes (placement, size class, colours and dot sizes are
  upstream's);
* ``select_subtype`` selects the rows whose ``motility_phenotype`` equals the subtype's code (0 immotile, 1 twitching,
  2 motile) -- upstream compares the NAME with that integer column and so selects nothing;
* interactive display (``output_save=False``) is not supported;
* the path of the written file is returned (upstream returns None either way); None still signals a failure.
"""
from __future__ import annotations

import logging
import os
import queue
import shutil
import struct
import threading
from fractions import Fraction

import numpy as np

from . import _lib
from .frames import DeviceFrameFeed, decode_mjpeg_setting, decode_tiff_setting, open_video
from .helper_file import create_results_folder, get_configs, get_data, get_loggers

__all__ = ["annotate_video", "AviWriter", "MjpegAviWriter", "DibOutput", "output_format", "jpeg_mode", "build_marks", "build_marks_device", "LAST_MARKS", "subtype_code", "SUBTYPES"]

SUBTYPES = ("immotile", "twitching", "motile")
#: one pinned output buffer (there are two) holds at most this many bytes
PINNED_BYTES_MAX = 256 << 20
#: what 'save video fourcc codec' may say without a warning: the names of an uncompressed stream
_RAW_CODECS = ("", "DIB ", "DIB", "RGB ", "RGB", "RAW ", "RAW", "0")
#: the names 'save video fourcc codec' has for Motion-JPEG (with 'save video file extension' = .avi)
_JPEG_CODECS = ("MJPG", "JPEG")
JPEG_QUALITY_DEFAULT = 90
#: the encoder's workspace (about 16 bytes per pixel of a batch at 4:4:4, 8 at 4:2:0) is kept at or below this by the batch size
MJPEG_WORKSPACE_MAX = 1 << 30
#: 'hip video jpeg subsampling' -> the ``sampling`` of ysmr_mjpeg_encode_batch; 'hip video jpeg huffman' -> its ``huffman``
JPEG_SUBSAMPLINGS = {"4:4:4": 1, "4:2:2": 2, "4:2:0": 3}
JPEG_HUFFMAN = {"standard": 0, "optimised": 1}


class AviWriter:
    """Uncompressed 24-bit AVI, written front to back and patched on ``close``.

    ``RIFF AVI`` (``hdrl``: ``avih``, ``strl`` with ``strh`` / ``strf``, ``odml`` with the total frame count; ``movi`` of
    ``00db`` chunks; ``idx1``) followed by ``RIFF AVIX`` segments (``movi`` only): a new segment is started whenever the
    next frame would take the current one past ``riff_limit`` bytes (a segment always holds at least one frame).  Frames
    are stored DIB frames: ``height`` rows of ``stride = (3 * width + 3) & ~3`` bytes, B, G, R per pixel, the last row
    first if ``bottom_up``.  ``strh``'s rate / scale are the best fraction for ``fps`` with a denominator of at most
    100000 (30000 / 1001 for 29.97...)."""

    HEADER_BYTES = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40)) + (12 + 8 + 4)) + 12      # up to and including 'movi'

    def __init__(self, path, width, height, fps, riff_limit=1 << 30, bottom_up=True):
        self.path, self.width, self.height, self.bottom_up = path, int(width), int(height), bool(bottom_up)
        self.stride = (3 * self.width + 3) & ~3
        self.frame_bytes = self.stride * self.height
        ratio = Fraction(float(fps)).limit_denominator(100000)
        if ratio <= 0:
            raise ValueError("fps must be positive, got {}".format(fps))
        self.rate, self.scale = ratio.numerator, ratio.denominator
        self.riff_limit = int(riff_limit)
        self.frames = 0
        self._first_frames = 0          # frames of the first segment: those of idx1 and avih
        self._index = []                # idx1 entries of the first segment
        self._fh = open(path, "wb")
        self._seg_start, self._movi_list, self._first = 0, self.HEADER_BYTES - 12, True
        self._fh.write(b"RIFF" + bytes(self.HEADER_BYTES - 16) + b"LIST" + bytes(4) + b"movi")   # (the rest on close)
        self._pos = self.HEADER_BYTES

    @staticmethod
    def file_bytes(width, height, n_frames, riff_limit=1 << 30):
        """Size of the file ``n_frames`` frames make: for the free-space check before writing."""
        frame = ((3 * int(width) + 3) & ~3) * int(height) + 8
        per_segment = max(1, (int(riff_limit) - AviWriter.HEADER_BYTES) // (frame + 16))
        segments = max(1, -(-int(n_frames) // per_segment))
        return AviWriter.HEADER_BYTES + n_frames * frame + 8 + 16 * min(n_frames, per_segment) + 24 * (segments - 1)

    def chunk_header(self):
        """The eight bytes in front of every frame."""
        return b"00db" + struct.pack("<I", self.frame_bytes)

    def _room(self):
        """How many more frames the current segment takes (at least one if it has none yet)."""
        used = self._pos - self._seg_start
        per = self.frame_bytes + 8 + (16 if self._first else 0)
        tail = 8 if self._first else 0                               # idx1's own header
        room = (self.riff_limit - used - tail) // per
        empty = self._pos == self._movi_list + 12
        return max(room, 1 if empty else 0)

    def _end_segment(self):
        fh = self._fh
        movi_size = self._pos - (self._movi_list + 8)
        if self._first:
            idx = self._idx1()
            fh.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
            self._pos += 8 + len(idx)
        fh.seek(self._movi_list + 4)
        fh.write(struct.pack("<I", movi_size))
        fh.seek(self._seg_start + 4)
        fh.write(struct.pack("<I", self._pos - (self._seg_start + 8)))
        fh.seek(self._pos)
        self._first = False

    def _idx1(self):
        return b"".join(struct.pack("<4sIII", b"00db", 0x10, off, self.frame_bytes) for off in self._index)

    def _stream_format(self):
        """(strh handler, biCompression, biHeight, bytes of the largest frame, bytes per second)."""
        size = self.frame_bytes
        return b"DIB ", 0, self.height if self.bottom_up else -self.height, size, int(size * self.rate / self.scale)

    def _new_segment(self):
        self._end_segment()
        self._seg_start, self._movi_list = self._pos, self._pos + 12
        self._fh.write(b"RIFF" + bytes(4) + b"AVIX" + b"LIST" + bytes(4) + b"movi")
        self._pos += 24

    def _note(self, n):
        if self._first:
            base = self._movi_list + 8                               # idx1 offsets count from the 'movi' fourcc
            self._index.extend(self._pos - base + k * (self.frame_bytes + 8) for k in range(n))
            self._first_frames += n
        self.frames += n
        self._pos += n * (self.frame_bytes + 8)

    def write(self, frames):
        """Append stored frames: a uint8 array [n, frame_bytes] (or anything that reshapes to it)."""
        frames = np.asarray(frames, dtype=np.uint8).reshape(-1, self.frame_bytes)
        head = self.chunk_header()
        for frame in frames:
            if self._room() < 1:
                self._new_segment()
            self._fh.write(head)
            self._fh.write(memoryview(np.ascontiguousarray(frame)))
            self._note(1)

    def write_chunks(self, chunks):
        """Append frames that already carry their chunk headers: a C-contiguous uint8 array [n, 8 + frame_bytes].  A run of
        frames that stays inside one segment is one write."""
        chunks = np.asarray(chunks)
        if chunks.dtype != np.uint8 or chunks.ndim != 2 or chunks.shape[1] != self.frame_bytes + 8 or not chunks.flags["C_CONTIGUOUS"]:
            raise ValueError("write_chunks needs a C-contiguous uint8 [n, {}] array".format(self.frame_bytes + 8))
        done = 0
        while done < len(chunks):
            room = self._room()
            if room < 1:
                self._new_segment()
                continue
            n = min(room, len(chunks) - done)
            self._fh.write(memoryview(chunks[done:done + n]).cast("B"))
            self._note(n)
            done += n

    def close(self):
        if self._fh is None:
            return
        fh = self._fh
        self._end_segment()
        handler, compression, bi_height, size, per_second = self._stream_format()
        avih = struct.pack("<14I", int(round(1e6 * self.scale / self.rate)), min(per_second, 0xFFFFFFFF), 0, 0x10,
                           self._first_frames, 0, 1, size, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", handler, 0, 0, 0, 0, self.scale, self.rate, 0, self.frames, size,
                           -1, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHHIIiiII", 40, self.width, bi_height, 1, 24, compression, size, 0, 0, 0, 0)

        def chunk(cid, body):
            return cid + struct.pack("<I", len(body)) + body

        def lst(kind, body):
            return chunk(b"LIST", kind + body)

        hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)) +
                   lst(b"odml", chunk(b"dmlh", struct.pack("<I", self.frames))))
        head = b"RIFF" + bytes(4) + b"AVI " + hdrl
        assert len(head) + 12 == self.HEADER_BYTES, len(head)
        fh.seek(8)                                                   # (the RIFF size and the movi LIST are in place)
        fh.write(head[8:])
        fh.close()
        self._fh = None

    def abort(self):
        """Close and remove the file."""
        if self._fh is not None:
            self._fh.close()
            self._fh = None
        try:
            os.remove(self.path)
        except OSError:
            pass


class MjpegAviWriter(AviWriter):
    """Motion-JPEG AVI: ``AviWriter``'s file with chunks of their own sizes.  ``strh`` handler and ``biCompression`` are
    ``MJPG`` (24 bits, positive height), the chunks are ``00dc``, every ``idx1`` entry carries its chunk's size, and
    ``biSizeImage`` / the suggested buffer size are the largest chunk's.  The segment rule (``RIFF AVIX``, ``riff_limit``),
    the rate / scale fraction and ``dmlh`` are ``AviWriter``'s."""

    def __init__(self, path, width, height, fps, riff_limit=1 << 30):
        super().__init__(path, width, height, fps, riff_limit=riff_limit, bottom_up=True)
        self._sizes = []                # payload sizes of the first segment's chunks, beside self._index
        self.largest = 0                # the largest payload
        self.payload_bytes = 0          # all payloads

    def _idx1(self):
        return b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in zip(self._index, self._sizes))

    def _stream_format(self):
        mean = self.payload_bytes / max(1, self.frames)
        return b"MJPG", struct.unpack("<I", b"MJPG")[0], self.height, self.largest, int(mean * self.rate / self.scale)

    def chunk_header(self):
        raise NotImplementedError("a Motion-JPEG chunk carries its own size")

    def write(self, frames):
        raise NotImplementedError("MjpegAviWriter takes finished chunks: write_chunks(data, offsets)")

    def write_chunks(self, data, offsets):
        """Append finished chunks: ``data`` a C-contiguous uint8 array with the chunks back to back ('00dc', the payload
        size, the payload, a zero byte if the size is odd), chunk i at ``data[offsets[i]:offsets[i + 1]]``.  A run of chunks
        that stays inside one segment is one write."""
        data = np.asarray(data)
        offsets = [int(o) for o in offsets]
        if data.dtype != np.uint8 or data.ndim != 1 or not data.flags["C_CONTIGUOUS"]:
            raise ValueError("write_chunks needs a C-contiguous one-dimensional uint8 array")
        if not offsets or offsets[-1] > len(data) or any(b - a < 8 for a, b in zip(offsets, offsets[1:])):
            raise ValueError("offsets {} do not describe chunks of an array of {} bytes".format(offsets, len(data)))
        sizes = []
        for a, b in zip(offsets, offsets[1:]):
            tag, size = struct.unpack_from("<4sI", data, a)
            if tag != b"00dc" or 8 + size + (size & 1) != b - a:
                raise ValueError("chunk at {}: tag {!r}, size {} in {} bytes".format(a, tag, size, b - a))
            sizes.append(size)
        done, n = 0, len(sizes)
        while done < n:
            run = done
            while run < n:                       # how many more chunks the current segment takes
                used = self._pos + (offsets[run] - offsets[done]) - self._seg_start
                more = offsets[run + 1] - offsets[run] + (16 * (len(self._index) + run - done + 1) + 8 if self._first else 0)
                empty = run == done and self._pos == self._movi_list + 12
                if used + more > self.riff_limit and not empty:
                    break
                run += 1
            if run == done:
                self._new_segment()
                continue
            self._fh.write(memoryview(data[offsets[done]:offsets[run]]))
            if self._first:
                base = self._movi_list + 8
                self._index.extend(self._pos - base + offsets[k] - offsets[done] for k in range(done, run))
                self._sizes.extend(sizes[done:run])
                self._first_frames += run - done
            self.frames += run - done
            self._pos += offsets[run] - offsets[done]
            self.largest = max([self.largest] + sizes[done:run])
            self.payload_bytes += sum(sizes[done:run])
            done = run


def jpeg_mode(settings):
    """``(sampling, huffman)`` for ``ysmr_mjpeg_encode_batch`` from the optional settings keys 'hip video jpeg subsampling'
    ('4:4:4', the default, '4:2:2' or '4:2:0') and 'hip video jpeg huffman' ('standard', the default, or 'optimised': tables
    built for every frame); ValueError, naming key and value, for anything else."""
    out = []
    for key, known in (("hip video jpeg subsampling", JPEG_SUBSAMPLINGS), ("hip video jpeg huffman", JPEG_HUFFMAN)):
        asked = settings.get(key)
        if asked is None or asked == "":
            out.append(next(iter(known.values())))
        elif isinstance(asked, str) and asked.strip().lower() in known:
            out.append(known[asked.strip().lower()])
        else:
            raise ValueError("{!r} must be one of {}, got {!r}".format(key, ", ".join(repr(k) for k in known), asked))
    return tuple(out)


def jpeg_mode_name(sampling, huffman):
    """'' for the default mode, else what the log says behind the quality: ', 4:2:0, optimised Huffman tables'."""
    parts = [name for name, code in JPEG_SUBSAMPLINGS.items() if code == sampling and code != 1]
    parts += ["{} Huffman tables".format(name) for name, code in JPEG_HUFFMAN.items() if code == huffman and code != 0]
    return "".join(", " + p for p in parts)


def output_format(settings):
    """What 'save video file extension' / 'save video fourcc codec' / 'hip video jpeg quality' ask for:
    ``(format, quality, warning)`` -- ``("mjpeg", 1 .. 100, None)`` exactly when the extension is ``.avi`` and the codec
    ``MJPG`` or ``JPEG`` (any letter case; the quality defaults to 90; ValueError if it is not 1 .. 100, or if
    'hip video jpeg subsampling' / 'hip video jpeg huffman' hold anything ``jpeg_mode`` does not know), else
    ``("raw", None, warning)`` with the warning (None for ``.avi`` and the name of an uncompressed stream) that the caller
    completes with the file name."""
    ext = str(settings.get("save video file extension") or "")
    codec = str(settings.get("save video fourcc codec") or "")
    if ext.lower() == ".avi" and codec.upper() in _JPEG_CODECS:
        asked = settings.get("hip video jpeg quality")
        try:
            quality = JPEG_QUALITY_DEFAULT if asked is None or asked == "" else int(asked)
        except (TypeError, ValueError):
            quality = None
        if quality is None or isinstance(asked, bool) or not 1 <= quality <= 100:
            raise ValueError("'hip video jpeg quality' must be an integer from 1 to 100, got {!r}".format(asked))
        jpeg_mode(settings)
        return "mjpeg", quality, None
    if ext.lower() != ".avi" or codec.upper() not in _RAW_CODECS:
        return "raw", None, ("'save video file extension' = {!r} / 'save video fourcc codec' = {!r}: the HIP path has no encoder; "
                             "writing an uncompressed 24-bit AVI instead".format(ext, codec))
    return "raw", None, None


def subtype_code(select_subtype):
    """0, 1, 2 for an int or one of 'immotile', 'twitching', 'motile'; ValueError otherwise."""
    if isinstance(select_subtype, str):
        if select_subtype.lower() not in SUBTYPES:
            raise ValueError("select_subtype must be 0, 1, 2 or one of {}, got {!r}".format(SUBTYPES, select_subtype))
        return SUBTYPES.index(select_subtype.lower())
    code = int(select_subtype)
    if code not in (0, 1, 2):
        raise ValueError("select_subtype must be 0, 1, 2 or one of {}, got {!r}".format(SUBTYPES, select_subtype))
    return code


def build_marks(df, n_frames, select_subtype=None):
    """The marks of a whole video from the evaluated table: ``(marks, first)`` -- ``marks`` a ``_lib.MARK_DTYPE`` array
    ordered by frame and, inside a frame, as in the table; the marks of frame i are ``marks[first[i]:first[i + 1]]``
    (``first``: int64 [n_frames + 1]).  x, y are POSITION_X / POSITION_Y truncated toward zero (``int()``, as upstream);
    rows with a position that is not finite or a POSITION_T outside [0, n_frames) are skipped; style 1 where ``moving``
    is 0, else 2 where ``turn_points`` is 1, else 0 (track_eval.py:1424-1432).  ``select_subtype``: keep the rows whose
    ``motility_phenotype`` is that subtype's code."""
    import pandas as pd
    x = df["POSITION_X"].to_numpy(dtype=np.float64)
    y = df["POSITION_Y"].to_numpy(dtype=np.float64)
    t = pd.to_numeric(df["POSITION_T"], errors="coerce").to_numpy(dtype=np.float64)
    keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(t)
    keep &= (np.where(keep, t, -1) >= 0) & (np.where(keep, t, -1) < n_frames)
    if select_subtype is not None:
        phenotype = pd.to_numeric(df["motility_phenotype"], errors="coerce").to_numpy(dtype=np.float64)
        keep &= phenotype == subtype_code(select_subtype)
    rows = np.flatnonzero(keep)
    frame = t[rows].astype(np.int64)
    order = np.argsort(frame, kind="stable")                         # table order survives inside a frame
    rows, frame = rows[order], frame[order]
    lim = np.iinfo(np.int32)
    marks = np.zeros(len(rows), _lib.MARK_DTYPE)
    marks["x"] = np.clip(np.trunc(x[rows]), lim.min, lim.max).astype(np.int32)
    marks["y"] = np.clip(np.trunc(y[rows]), lim.min, lim.max).astype(np.int32)
    marks["track_id"] = (df["TRACK_ID"].to_numpy()[rows].astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    moving = df["moving"].to_numpy()[rows]
    turn = df["turn_points"].to_numpy()[rows]
    marks["style"] = np.where(moving == 0, 1, np.where(turn == 1, 2, 0)).astype(np.uint32)
    first = np.searchsorted(frame, np.arange(n_frames + 1, dtype=np.int64), side="left").astype(np.int64)
    return marks, first


def auto_batch(chunk_bytes, n_frames):
    """Frames per batch: as many as keep one pinned output buffer at or below PINNED_BYTES_MAX."""
    return int(max(1, min(PINNED_BYTES_MAX // max(1, chunk_bytes), max(1, n_frames))))


def _csv_table(path, logger, settings):
    if settings["verbose"]:
        logger.debug("Handing string to get_data {}".format(path))
    dtype = {"TRACK_ID": np.int64, "POSITION_T": np.int64, "POSITION_X": np.float64, "POSITION_Y": np.float64,
             "motility_phenotype": object, "moving": np.int8, "turn_points": np.int8}
    return get_data(path, dtype=dtype)


#: which way the marks of the last ``annotate_video`` call came: "device" (csv read and marks built on the GPU), "host" (the
#: csv through pandas and ``build_marks``) or "frame" (a DataFrame argument); the rows of the table and the marks they gave
LAST_MARKS = {}
#: (diagnostics) seconds since ``annotate_video`` began at which its marks were on the device
LAST_MARKS_TIMES = {}


def _csv_fields(select_subtype):
    """The columns ``_csv_table`` reads, as the typed device reader takes them.  TRACK_ID as uint32: an id beyond it sends
    the file to pandas.  motility_phenotype only where it is looked at (its name has to be in the header either way)."""
    fields = [("TRACK_ID", np.uint32), ("POSITION_T", np.int64), ("POSITION_X", np.float64, True), ("POSITION_Y", np.float64, True),
              ("moving", np.int8), ("turn_points", np.int8)]
    if select_subtype is not None:
        fields.append(("motility_phenotype", np.float64, True))
    return fields


def build_marks_device(columns, n_rows, n_frames, select_subtype=None, sort_rule=2, device="cuda:0"):
    """``build_marks`` on the device (``ysmr_marks_build``, csrc/marks.hip): ``columns`` name -> tensor on ``device`` with
    TRACK_ID (32-bit), POSITION_T (int64), POSITION_X / POSITION_Y (float64), moving / turn_points (int8) and, with
    ``select_subtype``, motility_phenotype (float64, NaN where it is empty) -- what ``read_typed_device`` gives for
    ``_csv_fields``.  ``sort_rule``: what "table order" means -- 0 the order of the rows, 1 sorted by (TRACK_ID, POSITION_T),
    2 (``get_data``'s) the latter when upstream's rough check on the first six ids says so.  Returns ``(marks_dev,
    first_dev)``: uint8 [16 * n_rows] holding the marks (zeros behind the last one) and int64 [n_frames + 1], the same bytes
    as ``build_marks``' arrays; None where the library refuses the sizes.  Nothing waits for the device."""
    import torch
    L = _lib.lib()
    dev = torch.device(device)
    n_rows, n_frames = int(n_rows), int(n_frames)
    subtype = -1 if select_subtype is None else subtype_code(select_subtype)
    ws_bytes = int(L.ysmr_marks_workspace_bytes(n_rows, n_frames)) if 0 < n_frames < 2 ** 31 else 0
    if ws_bytes == 0:
        return None
    wanted = {"TRACK_ID": 4, "POSITION_T": 8, "POSITION_X": 8, "POSITION_Y": 8, "moving": 1, "turn_points": 1}
    if select_subtype is not None:
        wanted["motility_phenotype"] = 8
    pointers = []
    for name, size in wanted.items():
        col = columns[name]
        if col.device != dev or not col.is_contiguous() or col.element_size() != size or col.numel() < n_rows:
            raise ValueError("column {!r}: {} contiguous values of {} bytes on {} are needed".format(name, n_rows, size, dev))
        pointers.append(col.data_ptr() if n_rows else 0)
    if select_subtype is None:
        pointers.append(0)
    with _lib.on(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        marks_dev = torch.empty(max(16 * n_rows, 16), dtype=torch.uint8, device=dev)
        first_dev = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
        _lib.check(L.ysmr_marks_build(_lib.stream_ptr(dev), n_rows, *pointers, subtype, n_frames, int(sort_rule), ws.data_ptr(), ws_bytes,
                                      marks_dev.data_ptr(), first_dev.data_ptr()), "ysmr_marks_build")
    return marks_dev, first_dev


class DibOutput:
    """The way of painted frames from the device to the file, for ``annotate_video`` and for the detection view of
    ``track_bacteria``: two slots, each a device buffer of ``batch`` stored DIB frames and a pinned host buffer, a copy
    stream and a writer thread.

    ``writer`` an ``AviWriter``: every frame has its chunk header in front of it, written once here (the kernels write
    behind it), so that a batch goes to the file as it is.  A ``MjpegAviWriter`` (``quality`` and ``mode``, its sampling
    and huffman, are then needed): ``ysmr_mjpeg_encode_batch`` encodes a slot's frames into finished chunks, the copy stream
    brings the offsets and the status over and then only the bytes the offsets name; the output buffers' default capacity
    is the batch's uncompressed size, and a batch that does not fit is encoded once more into buffers of the size its
    offsets ask for; the free space of ``result_folder`` is checked against the bytes about to be written.

    ``acquire`` -> a slot whose last batch has been written; ``frames`` -> where a kernel paints it; ``submit`` hands its
    first n frames over once ``painted`` (an event) has happened; ``close`` waits for the writer thread.  A failure of the
    writer thread is raised by the next ``acquire``; after ``close`` it is in ``failure``.  ``submit`` and ``close`` make
    ``dev`` the current device themselves.  ``dib_slots`` (Motion-JPEG only, where the frames are painted into a DIB buffer
    and encoded from there): 1 -- paint and encode of a batch follow each other on one stream, as in ``annotate_video``, and
    one buffer serves both slots; 2 -- a buffer per slot, for a caller that paints a batch while the one before still waits
    to be encoded (the detection view)."""

    def __init__(self, writer, batch, height, width, dev, quality=None, mode=None, result_folder=None, logger=None, dib_slots=1):
        import torch
        self.writer, self.batch, self.dev, self.height, self.width = writer, int(batch), dev, int(height), int(width)
        self.mjpeg = isinstance(writer, MjpegAviWriter)
        self.logger, self.result_folder = logger, result_folder
        self.shortfall = None              # (bytes needed, bytes free) once the disk has run full: nothing more is written
        self.L = _lib.lib()
        frame_bytes = writer.frame_bytes
        with _lib.on(dev):
            if self.mjpeg:
                self.quality, (self.sampling, self.huffman) = quality, mode
                self.ws_bytes = self.L.ysmr_mjpeg_encode_workspace_bytes(self.batch, self.height, self.width, self.sampling, self.huffman)
                if not self.ws_bytes:
                    raise ValueError("a Motion-JPEG frame is at most 65535 x 65535, got {} x {}".format(width, height))
                self.pitch = frame_bytes
                self.dib = [torch.empty((self.batch, frame_bytes), dtype=torch.uint8, device=dev) for _k in range(2 if dib_slots > 1 else 1)]
                self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
                self.capacity = [self.batch * frame_bytes] * 2
                self.out_dev = [torch.empty(self.capacity[k], dtype=torch.uint8, device=dev) for k in range(2)]
                self.pinned = [torch.empty(self.capacity[k], dtype=torch.uint8, pin_memory=True) for k in range(2)]
                # offsets [batch + 1] and, in the last element, the status
                self.meta_dev = [torch.zeros(self.batch + 2, dtype=torch.int64, device=dev) for _k in range(2)]
                self.meta = [torch.zeros(self.batch + 2, dtype=torch.int64, pin_memory=True) for _k in range(2)]
            else:
                self.pitch = frame_bytes + 8
                head = torch.from_numpy(np.frombuffer(writer.chunk_header(), np.uint8).copy())
                self.out_dev, self.pinned = [], []
                for _k in range(2):
                    buf = torch.empty((self.batch, self.pitch), dtype=torch.uint8, device=dev)
                    buf[:, :8] = head.to(dev)
                    self.out_dev.append(buf)
                    self.pinned.append(torch.empty((self.batch, self.pitch), dtype=torch.uint8, pin_memory=True))
            self.copy_stream = torch.cuda.Stream(device=dev)
        self.free_slots, self.jobs, self.failure = queue.Queue(), queue.Queue(), []
        for k in range(2):
            self.free_slots.put(k)
        self.thread = threading.Thread(target=self._write_loop, name="ysmr-annotate-writer", daemon=True)
        self.thread.start()

    @staticmethod
    def mjpeg_batch_limit(height, width, mode):
        """The most frames per batch that keep the encoder's workspace at or below MJPEG_WORKSPACE_MAX."""
        return max(1, MJPEG_WORKSPACE_MAX // max(1, _lib.lib().ysmr_mjpeg_encode_workspace_bytes(1, height, width, mode[0], mode[1])))

    def _write_loop(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            k, what, copied = job
            try:
                if not self.failure:
                    copied.synchronize()
                    if self.mjpeg:
                        self.writer.write_chunks(self.pinned[k].numpy()[:what[-1]], what)
                    else:
                        self.writer.write_chunks(self.pinned[k].numpy()[:what])
            except BaseException as exc:      # noqa: BLE001 -- handed to the caller's thread
                self.failure.append(exc)
            self.free_slots.put(k)

    def acquire(self):
        k = self.free_slots.get()              # its last copy has been written: both buffers of slot k are free
        if self.failure:
            raise self.failure[0]
        return k

    def frames(self, k):
        """(device pointer of the slot's first stored frame, bytes from one frame to the next)."""
        return (self.dib[k % len(self.dib)].data_ptr(), self.pitch) if self.mjpeg else (self.out_dev[k].data_ptr() + 8, self.pitch)

    def _encode(self, stream, k, n):
        """Encode the painted batch into slot k and bring offsets and status over: (offsets, status)."""
        import torch
        w = self.writer
        _lib.check(self.L.ysmr_mjpeg_encode_batch(
            stream.cuda_stream, self.dib[k % len(self.dib)].data_ptr(), n, self.height, self.width, w.stride, w.frame_bytes, int(w.bottom_up),
            self.quality, self.sampling, self.huffman, self.workspace.data_ptr(), self.ws_bytes, self.out_dev[k].data_ptr(),
            self.capacity[k], self.meta_dev[k].data_ptr(), self.meta_dev[k].data_ptr() + 8 * (self.batch + 1)), "ysmr_mjpeg_encode_batch")
        encoded = torch.cuda.Event()
        encoded.record(stream)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(encoded)
            self.meta[k].copy_(self.meta_dev[k], non_blocking=True)
            known = torch.cuda.Event()
            known.record(self.copy_stream)
        known.synchronize()
        values = self.meta[k].numpy()
        return [int(v) for v in values[:n + 1]], int(values[self.batch + 1]) & 0xFFFFFFFF

    def submit(self, k, n, first_frame, stream, painted):
        """The first ``n`` frames of slot k, painted on ``stream`` (``painted``: an event recorded there behind the paint),
        are frames ``first_frame`` .. of the file.  False: the disk is full (``shortfall``), nothing was handed over."""
        with _lib.on(self.dev):
            return self._submit(k, n, first_frame, stream, painted)

    def _submit(self, k, n, first_frame, stream, painted):
        import torch
        if not self.mjpeg:
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(painted)
                self.pinned[k][:n].copy_(self.out_dev[k][:n], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(self.copy_stream)
            self.jobs.put((k, n, copied))
            return True
        offsets, status = self._encode(stream, k, n)
        if status & 1:
            if self.logger is not None:
                self.logger.debug("Motion-JPEG: frames {} .. {} take {} bytes, the buffer has {}: encoding them again".format(
                    first_frame, first_frame + n - 1, offsets[-1], self.capacity[k]))
            self.capacity[k] = offsets[-1]
            self.out_dev[k] = torch.empty(self.capacity[k], dtype=torch.uint8, device=self.dev)
            self.pinned[k] = torch.empty(self.capacity[k], dtype=torch.uint8, pin_memory=True)
            offsets, status = self._encode(stream, k, n)
        if status:
            raise RuntimeError("ysmr_mjpeg_encode_batch: status {} for frames {} .. {} ({} bytes into {})".format(
                status, first_frame, first_frame + n - 1, offsets[-1], self.capacity[k]))
        need, free = offsets[-1] + 24 * n + 4096, shutil.disk_usage(self.result_folder).free
        if free < need:
            self.shortfall = (need, free)
            self.free_slots.put(k)
            return False
        with torch.cuda.stream(self.copy_stream):
            self.pinned[k][:offsets[-1]].copy_(self.out_dev[k][:offsets[-1]], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self.copy_stream)
        self.jobs.put((k, offsets, copied))
        return True

    def close(self):
        """Wait for everything handed over to be written (or given up); safe to call twice."""
        import torch
        if self.thread is not None:
            self.jobs.put(None)
            self.thread.join()
            self.thread = None
            with _lib.on(self.dev):
                torch.cuda.synchronize(self.dev)


def enough_space(result_folder, needed, what, logger):
    """The free-space check in front of an uncompressed file: False after a critical message."""
    free = shutil.disk_usage(result_folder).free
    if free < needed:
        logger.critical("Not enough free space in {} for the {}: {} bytes needed, {} free".format(result_folder, what, needed, free))
        return False
    return True


def annotate_video(video_path, df, output_save=True, settings=None, result_folder=None, select_subtype=None,
                   device="cuda:0", **_):
    """Write ``<name>_annotated_output.avi`` (``<subtype>_subtype_<name>_annotated_output.avi`` with ``select_subtype``)
    into ``result_folder``: the video with every track's id and centroid painted into the frames of the table ``df`` (the
    first element of ``evaluate_tracks``' result, or the path of an ``*_analysed.csv``) -- green, orange where the track is
    not moving, white with a larger dot at turn points.  Returns the path of the file, None after any failure (logged on
    'ysmr', never raised).  Optional settings keys: 'hip frames per batch' overrides the batch size; 'hip video jpeg
    quality' (1 .. 100, default 90) is the quality of a Motion-JPEG file (``output_format`` says when one is written;
    the free space is then checked batch by batch, against the bytes about to be written), 'hip video jpeg subsampling'
    ('4:4:4' / '4:2:2' / '4:2:0') and 'hip video jpeg huffman' ('standard' / 'optimised') its chroma subsampling and
    whether every frame carries Huffman tables of its own (``jpeg_mode``); 'hip decode mjpeg' (True /
    'always' / False) says whether a Motion-JPEG INPUT is decoded on the device, and 'hip decode tiff' (True / False) whether a
    TIFF stack is, as in ``track_bacteria``; a true 'hip read
    csv on device' reads a csv ``df`` and builds its marks on the device (``read_typed_device``, ``build_marks_device``) --
    the same file; a csv the device reader does not serve is read by pandas as without the key.  ``LAST_MARKS`` says which
    way the call went."""
    import time
    import pandas as pd
    import torch
    started = time.perf_counter()
    LAST_MARKS.clear()
    LAST_MARKS_TIMES.clear()
    logger = logging.getLogger("ysmr").getChild(__name__)
    settings = get_configs(settings)
    if settings is None:
        logger.critical("No settings provided / could not get settings for annotate_video().")
        return None
    get_loggers(log_level=settings["log_level"], logfile_name=settings["log file path"],
                short_stream_output=settings["shorten displayed logging output"],
                short_file_output=settings["shorten logfile logging output"], log_to_file=settings["log to file"])
    if not output_save:
        logger.critical("output_save = False (interactive display) is not supported by the HIP path")
        return None
    try:
        video = open_video(video_path, default_fps=settings["frames per second"])
    except (OSError, ValueError) as exc:
        logger.exception("Cannot open file {} due to error: {}".format(video_path, exc))
        return None
    writer = feed = None
    try:
        if not result_folder:
            result_folder = create_results_folder(video_path)
        os.makedirs(result_folder, exist_ok=True)
        csv_path = typed = None
        if not isinstance(df, pd.DataFrame):
            csv_path = df
            if settings.get("hip read csv on device"):
                # (a file the device reader does not serve is read by pandas, here, as without the key)
                from .helper_file import read_typed_device
                typed = read_typed_device(csv_path, _csv_fields(select_subtype), torch.device(device), also_in_header=("motility_phenotype",))
                typed = typed if typed.path_taken == "device" else None
            if typed is None:
                df = _csv_table(csv_path, logger, settings)
                if df is None:
                    return None

        def table_marks():
            """(marks, first) of the table: tensors from the device path, arrays from the host's; None as ``_csv_table``."""
            nonlocal df
            if typed is not None:
                built = build_marks_device(typed.columns, typed.n_rows, n_frames, select_subtype, sort_rule=2, device=dev)
                if built is not None:
                    LAST_MARKS.update(path="device", rows=typed.n_rows)
                    return built
                df = _csv_table(csv_path, logger, settings)
                if df is None:
                    return None
            LAST_MARKS.update(path="frame" if csv_path is None else "host", rows=len(df))
            return build_marks(df, n_frames, select_subtype)
        fps_of_file = video.fps
        if not fps_of_file or not fps_of_file > 0:
            if settings["frames per second"] <= 0:
                logger.critical("User defined fps unacceptable: type: {} value: {}".format(
                    type(settings["frames per second"]), settings["frames per second"]))
                return None
            fps_of_file = settings["frames per second"]
        filename = os.path.splitext(os.path.basename(video_path))[0]
        if select_subtype is None:
            name = "{}_annotated_output.avi".format(filename)
        else:
            select_subtype = subtype_code(select_subtype)
            name = "{}_subtype_{}_annotated_output.avi".format(SUBTYPES[select_subtype], filename)
        output_video_name = os.path.join(result_folder, name)
        try:
            fmt, quality, warning = output_format(settings)
        except ValueError as exc:
            logger.critical(str(exc))
            return None
        if warning:
            logger.warning("{}: {}".format(warning, output_video_name))
        held = getattr(video, "frames_available", video.frame_count)
        n_frames = int(held if held < (1 << 60) else video.frame_count)
        if n_frames <= 0:
            logger.critical("Error during cap.read() with file {}".format(video_path))
            return None
        height, width, channels = video.height, video.width, video.channels
        dev = torch.device(device)
        L = _lib.lib()
        if fmt == "mjpeg":
            built = table_marks()
            if built is None:
                return None
            writer = MjpegAviWriter(output_video_name, width, height, fps_of_file)
            mode = jpeg_mode(settings)
            logger.info("Annotated video {}: {} frames of {} x {}, Motion-JPEG, quality {}{}".format(
                output_video_name, n_frames, width, height, quality, jpeg_mode_name(*mode)))
            batch = int(settings.get("hip frames per batch") or 0) or auto_batch(writer.frame_bytes + 8, n_frames)
            batch = max(1, min(batch, auto_batch(writer.frame_bytes + 8, n_frames), DibOutput.mjpeg_batch_limit(height, width, mode)))
        else:
            mode = None
            expected = AviWriter.file_bytes(width, height, n_frames)
            logger.info("Annotated video {}: {} frames of {} x {}, {:.1f} MiB uncompressed".format(
                output_video_name, n_frames, width, height, expected / 2 ** 20))
            if not enough_space(result_folder, expected, "annotated video", logger):
                return None
            built = table_marks()
            if built is None:
                return None
            writer = AviWriter(output_video_name, width, height, fps_of_file)
            batch = int(settings.get("hip frames per batch") or 0) or auto_batch(writer.frame_bytes + 8, n_frames)
            batch = max(1, min(batch, auto_batch(writer.frame_bytes + 8, n_frames)))
        sink = DibOutput(writer, batch, height, width, dev, quality=quality, mode=mode, result_folder=result_folder, logger=logger)
        done = 0
        try:
            with _lib.on(dev):
                if LAST_MARKS["path"] == "device":
                    marks_dev, first_dev = built
                    LAST_MARKS["marks"] = int(first_dev[-1:].cpu()[0])
                else:
                    marks, first = built
                    marks_dev = torch.from_numpy(marks.view(np.uint8).reshape(-1)).to(dev) if len(marks) else \
                        torch.zeros(16, dtype=torch.uint8, device=dev)
                    first_dev = torch.from_numpy(first).to(dev)
                    LAST_MARKS["marks"] = len(marks)
                LAST_MARKS_TIMES["marks on device"] = time.perf_counter() - started
                feed = DeviceFrameFeed(video, batch, dev, depth=2, decode_on_device=decode_mjpeg_setting(settings),
                                       decode_tiff=decode_tiff_setting(settings))
                for frames_dev, f0, n, slot in feed:
                    n = min(n, n_frames - f0)
                    if n <= 0:
                        feed.release(slot, True)
                        break
                    k = sink.acquire()
                    stream = torch.cuda.current_stream(dev)
                    out_ptr, pitch = sink.frames(k)
                    _lib.check(L.ysmr_annotate_batch(
                        stream.cuda_stream, frames_dev.data_ptr(), n, height, width, channels, marks_dev.data_ptr(),
                        first_dev.data_ptr() + 8 * f0, out_ptr, writer.stride, pitch, int(writer.bottom_up)), "ysmr_annotate_batch")
                    painted = torch.cuda.Event()
                    painted.record(stream)
                    feed.release(slot, painted)
                    if not sink.submit(k, n, f0, stream, painted):
                        break
                    done = f0 + n
        finally:
            with _lib.on(dev):
                sink.close()
        if sink.failure:
            raise sink.failure[0]
        if sink.shortfall:
            logger.critical("Not enough free space in {} for the annotated video: {} bytes needed, {} free".format(
                result_folder, sink.shortfall[0], sink.shortfall[1]))
            return None
        frame_count = video.frame_count
        if done not in (frame_count, frame_count - 1):   # (track_eval.py:1411-1418: some formats report one frame more)
            logger.critical("Error during cap.read() with file {}".format(video_path))
        else:
            logger.debug("Frames from file {} read.".format(os.path.basename(video_path)))
        writer.close()
        writer = None
        if fmt == "mjpeg":
            written, raw = os.path.getsize(output_video_name), AviWriter.file_bytes(width, height, done)
            logger.info("Output video file: {}: {:.1f} MiB written, {:.3f} of the {:.1f} MiB of the uncompressed AVI".format(
                output_video_name, written / 2 ** 20, written / raw, raw / 2 ** 20))
        else:
            logger.debug("Output video file: {}".format(output_video_name))
        return output_video_name
    except Exception as exc:      # noqa: BLE001 -- "log + return None", as every entry point
        logger.critical("Annotating file {} failed: {}: {}".format(video_path, type(exc).__name__, exc))
        return None
    finally:
        if feed is not None:
            feed.close()
        if writer is not None:
            writer.abort()
        video.close()
