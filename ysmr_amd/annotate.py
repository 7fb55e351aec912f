"""``annotate_video`` -- the annotated output video on the device (ysmr/track_eval.py:1321-1472).

Upstream reads the video again, paints every track's id and centroid into each frame (``cv2.putText``, ``cv2.circle``)
and hands the frames to ``cv2.VideoWriter``.  Here the frames come through ``DeviceFrameFeed``, ``ysmr_annotate_batch``
(``csrc/annotate.hip``) paints the marks and lays the frames out as stored 24-bit DIB frames, a stream of its own copies
them into one of two pinned buffers, and a writer thread appends those to an uncompressed AVI (``AviWriter``): the host
moves bytes and touches no pixel.

Departures from upstream, all deliberate:

* the file is always an uncompressed 24-bit ``.avi`` (no encoder is a dependency of this package); settings that ask for
  another container or codec are answered with one warning that names what is written;
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
from .frames import DeviceFrameFeed, open_video
from .helper_file import create_results_folder, get_configs, get_data, get_loggers

__all__ = ["annotate_video", "AviWriter", "build_marks", "subtype_code", "SUBTYPES"]

SUBTYPES = ("immotile", "twitching", "motile")
#: one pinned output buffer (there are two) holds at most this many bytes
PINNED_BYTES_MAX = 256 << 20
#: what 'save video fourcc codec' may say without a warning: the names of an uncompressed stream
_RAW_CODECS = ("", "DIB ", "DIB", "RGB ", "RGB", "RAW ", "RAW", "0")


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
            idx = b"".join(struct.pack("<4sIII", b"00db", 0x10, off, self.frame_bytes) for off in self._index)
            fh.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
            self._pos += 8 + len(idx)
        fh.seek(self._movi_list + 4)
        fh.write(struct.pack("<I", movi_size))
        fh.seek(self._seg_start + 4)
        fh.write(struct.pack("<I", self._pos - (self._seg_start + 8)))
        fh.seek(self._pos)
        self._first = False

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
        size = self.frame_bytes
        avih = struct.pack("<14I", int(round(1e6 * self.scale / self.rate)), min(int(size * self.rate / self.scale), 0xFFFFFFFF), 0, 0x10,
                           self._first_frames, 0, 1, size, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", b"DIB ", 0, 0, 0, 0, self.scale, self.rate, 0, self.frames, size,
                           -1, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHHIIiiII", 40, self.width, self.height if self.bottom_up else -self.height, 1, 24, 0, size,
                           0, 0, 0, 0)

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


def annotate_video(video_path, df, output_save=True, settings=None, result_folder=None, select_subtype=None,
                   device="cuda:0", **_):
    """Write ``<name>_annotated_output.avi`` (``<subtype>_subtype_<name>_annotated_output.avi`` with ``select_subtype``)
    into ``result_folder``: the video with every track's id and centroid painted into the frames of the table ``df`` (the
    first element of ``evaluate_tracks``' result, or the path of an ``*_analysed.csv``) -- green, orange where the track is
    not moving, white with a larger dot at turn points.  Returns the path of the file, None after any failure (logged on
    'ysmr', never raised).  Optional settings key 'hip frames per batch' overrides the batch size."""
    import pandas as pd
    import torch
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
        if not isinstance(df, pd.DataFrame):
            df = _csv_table(df, logger, settings)
            if df is None:
                return None
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
        asked_ext = str(settings.get("save video file extension") or "")
        asked_codec = str(settings.get("save video fourcc codec") or "")
        if asked_ext.lower() != ".avi" or asked_codec.upper() not in _RAW_CODECS:
            logger.warning("'save video file extension' = {!r} / 'save video fourcc codec' = {!r}: the HIP path has no encoder; "
                           "writing an uncompressed 24-bit AVI instead: {}".format(asked_ext, asked_codec, output_video_name))
        held = getattr(video, "frames_available", video.frame_count)
        n_frames = int(held if held < (1 << 60) else video.frame_count)
        if n_frames <= 0:
            logger.critical("Error during cap.read() with file {}".format(video_path))
            return None
        height, width, channels = video.height, video.width, video.channels
        expected = AviWriter.file_bytes(width, height, n_frames)
        logger.info("Annotated video {}: {} frames of {} x {}, {:.1f} MiB uncompressed".format(
            output_video_name, n_frames, width, height, expected / 2 ** 20))
        free = shutil.disk_usage(result_folder).free
        if free < expected:
            logger.critical("Not enough free space in {} for the annotated video: {} bytes needed, {} free".format(
                result_folder, expected, free))
            return None
        marks, first = build_marks(df, n_frames, select_subtype)
        writer = AviWriter(output_video_name, width, height, fps_of_file)
        chunk_bytes = writer.frame_bytes + 8
        batch = int(settings.get("hip frames per batch") or 0) or auto_batch(chunk_bytes, n_frames)
        batch = max(1, min(batch, auto_batch(chunk_bytes, n_frames)))
        dev = torch.device(device)
        L = _lib.lib()
        with _lib.on(dev):
            marks_dev = torch.from_numpy(marks.view(np.uint8).reshape(-1)).to(dev) if len(marks) else \
                torch.zeros(16, dtype=torch.uint8, device=dev)
            first_dev = torch.from_numpy(first).to(dev)
            # two output buffers on the device and two pinned ones; every frame has its chunk header in front of it, written
            # once here (the kernels write behind it), so that a batch goes to the file as it is
            head = torch.from_numpy(np.frombuffer(writer.chunk_header(), np.uint8).copy())
            out_dev, pinned = [], []
            for _k in range(2):
                buf = torch.empty((batch, chunk_bytes), dtype=torch.uint8, device=dev)
                buf[:, :8] = head.to(dev)
                out_dev.append(buf)
                pinned.append(torch.empty((batch, chunk_bytes), dtype=torch.uint8, pin_memory=True))
            copy_stream = torch.cuda.Stream(device=dev)
            free_slots, jobs, failure = queue.Queue(), queue.Queue(), []
            for k in range(2):
                free_slots.put(k)

            def write_loop():
                while True:
                    job = jobs.get()
                    if job is None:
                        return
                    k, n, copied = job
                    try:
                        if not failure:
                            copied.synchronize()
                            writer.write_chunks(pinned[k].numpy()[:n])
                    except BaseException as exc:      # noqa: BLE001 -- handed to the caller's thread
                        failure.append(exc)
                    free_slots.put(k)

            thread = threading.Thread(target=write_loop, name="ysmr-annotate-writer", daemon=True)
            thread.start()
            done = 0
            try:
                feed = DeviceFrameFeed(video, batch, dev, depth=2)
                for frames_dev, f0, n, slot in feed:
                    n = min(n, n_frames - f0)
                    if n <= 0:
                        feed.release(slot, True)
                        break
                    k = free_slots.get()              # its last copy has been written: both buffers of slot k are free
                    if failure:
                        raise failure[0]
                    stream = torch.cuda.current_stream(dev)
                    _lib.check(L.ysmr_annotate_batch(
                        stream.cuda_stream, frames_dev.data_ptr(), n, height, width, channels, marks_dev.data_ptr(),
                        first_dev.data_ptr() + 8 * f0, out_dev[k].data_ptr() + 8, writer.stride, chunk_bytes,
                        int(writer.bottom_up)), "ysmr_annotate_batch")
                    painted = torch.cuda.Event()
                    painted.record(stream)
                    feed.release(slot, painted)
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(painted)
                        pinned[k][:n].copy_(out_dev[k][:n], non_blocking=True)
                        copied = torch.cuda.Event()
                        copied.record(copy_stream)
                    jobs.put((k, n, copied))
                    done = f0 + n
            finally:
                jobs.put(None)
                thread.join()
                torch.cuda.synchronize(dev)
            if failure:
                raise failure[0]
        frame_count = video.frame_count
        if done not in (frame_count, frame_count - 1):   # (track_eval.py:1411-1418: some formats report one frame more)
            logger.critical("Error during cap.read() with file {}".format(video_path))
        else:
            logger.debug("Frames from file {} read.".format(os.path.basename(video_path)))
        writer.close()
        writer = None
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
