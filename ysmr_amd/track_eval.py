"""``track_bacteria`` -- the per-frame detect-and-link loop of YSMR on the GPU.

Same contract as ``ysmr.track_eval.track_bacteria`` (ysmr/track_eval.py:38-405): given a video
path and the tracking.ini settings it writes ``<name>_list.csv`` and returns
``(DataFrame, fps, frame_height, frame_width, csv_path)``, or ``None`` after logging the reason.
The loop body (track_eval.py:156-366) is replaced by batched device work:

    frames (host) --H2D--> ysmr_detect_batch  (threshold, hysteresis, components, minAreaRect)
                           ysmr_tracker_run   (claims, lifecycle, GSFF, rows; state stays in HBM)
                     <--D2H-- rows, every `list save length interval` rows

Detection of batch b+1 is issued on a second HIP stream while batch b is being linked.

'include luminosity in tracking calculation' (track_eval.py:290-300; with 'disable gsff' = True, the combination upstream
runs): ``ysmr_luminosity_batch`` follows the detection on that stream and the link is ``ysmr_tracker_run3`` in link mode
2 -- one launch per batch (k_batch3) for the default shapes, one per frame otherwise -- with the mean gray value under each
detection's box as a third coordinate.
"""
from __future__ import annotations

import logging
import os
import gc
import itertools
import threading
import time

import numpy as np
import torch

from . import _lib
from ._lib import on_own_device
from .detect import Detector, MeanGrayState, mean_gray_params, threshold_params
from .frames import DeviceFrameFeed, decode_mjpeg_setting, decode_tiff_setting, open_video
from .helper_file import (COLOR_BGR2GRAY, RowStream, create_results_folder, get_configs, get_loggers, rows_to_csv_bytes, rows_to_csv_file, rows_to_csv_file_and_dataframe, rows_device_to_csv_file_and_dataframe,
                          rows_to_dataframe, save_list, wait_for_removals)
from .tracker import DeviceTracker, rows_to_numpy, sort_rows

__all__ = ["track_bacteria", "TrackingPipeline", "select_tracks", "evaluate_tracks", "annotate_video", "detection_video_path",
           "threshold_video_path", "threshold_view_mode"]

#: where the wall time of the last _device_pass went, in seconds since it began (diagnostics: scripts/e2e_profile.py)
LAST_PASS_MARKS = {}
#: which device buffers and which link path the last _device_pass ran with (the re-run of a video too dense for its first attempt)
LAST_PIPELINE_FACTS = {}

#: most rows kept on the device for one video (40 B each); longer tables are moved to the host in between
ROW_BUDGET_MAX = 32 << 20


def __getattr__(name):   # select_tracks / evaluate_tracks / annotate_video live in track_eval upstream (track_eval.py:536, 846, 1321)
    if name == "annotate_video":
        from .annotate import annotate_video
        return annotate_video
    if name == "select_tracks":
        from .select import select_tracks
        return select_tracks
    if name == "evaluate_tracks":
        from .evaluate import evaluate_tracks
        return evaluate_tracks
    raise AttributeError(name)


class HostRows:
    """A video's rows, ordered, in a NumPy array.  Like ``DeviceRows`` and ``RowStream`` a finished table: ``len()``,
    ``finish(path)`` -> (bytes of csv, DataFrame) with the csv written to ``path``, no file for None, and ``close()``."""

    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def finish(self, path=None):
        # the csv and the DataFrame's columns come out of ONE native pass over the rows (the values the text is printed from are
        # the values pandas would read back from it: worked out once, by the formatting threads themselves)
        if path is not None:
            return rows_to_csv_file_and_dataframe(self.rows, path)
        return 0, rows_to_dataframe(self.rows)

    def close(self):
        pass


class DeviceRows:
    """A video's rows, ordered, still on the device (``TrackingPipeline.take_rows_device``): the same finished table."""

    def __init__(self, rows_u8, count):
        self.rows_u8, self.count = rows_u8, int(count)

    def __len__(self):
        return self.count

    def finish(self, path=None):
        # Round 5: text and columns come from the device, where the ordered rows are (shortest digits, CPython's layout, pandas'
        # reading: csrc/fmt.h) -- the host copies them over and writes the file.  A table with a value the device form does not
        # print (none that a track produces) is brought over and takes the host path.
        made = rows_device_to_csv_file_and_dataframe(self.rows_u8, self.count, path)
        return made if made is not None else HostRows(rows_to_numpy(self.rows_u8, self.count)).finish(path)

    def close(self):
        pass


class TrackingPipeline:
    """Device-resident detect+link over consecutive batches of one video stream: ``detect_async`` issues a batch's detection
    on a side stream (two detectors ping-pong), ``link`` its 64 link launches on the caller's stream, ``take_rows`` hands
    the rows over (ordered on the device with ``sort=True``).  Rows accumulate in ``self.rows`` (``rows_per_flush`` of
    them); ``track_bacteria`` empties the buffer when it fills and -- with the optional settings key 'hip persist rows' --
    appends every full buffer to ``<name>_list.csv`` as the reference does, so that an interrupted run keeps what was
    tracked.  ``link=False``: detection only (no tracker neighbour: the matrix-pipe threshold kernel is used)."""

    def __init__(self, height, width, fps, settings, batch=64, max_det=2048, capacity=768, device="cuda:0",
                 rows_per_flush=None, link=True):
        self.device = torch.device(device)
        self.B = int(batch)
        offset = settings["threshold offset for detection"]
        mean_state = None
        if settings["adaptive double threshold"] < 0:
            # mean-gray branch (track_eval.py:219-253): the moving average runs through the video, so
            # both detectors share its state (their launches are ordered on the side stream)
            params = mean_gray_params(settings["white bacteria on dark background"], offset, fps)
            mean_state = MeanGrayState(params.window, self.device)
        else:
            params = threshold_params(settings["white bacteria on dark background"], offset,
                                      settings["adaptive double threshold"])
        # two detectors: batch b+1 is detected (stream 1) while batch b is linked (stream 0)
        # optional settings key 'opencv version' ('4.5.0', '4.10.0', '3.4.18', ...): which release the BGR2GRAY
        # coefficients and the minAreaRect angle convention follow (include/ysmr_hip.h: cv_flavour)
        # Which threshold kernel: detection of batch b+1 runs BESIDE the link of batch b, and there the float32-chain strip
        # kernel is the better neighbour -- its resident grid leaves a wave slot, registers and LDS on every compute unit
        # for the link's chain of 10 us kernels, while the matrix-pipe kernel takes whole units (160 KB of LDS, every
        # register) and the link waits for them: 80.7 k against 85.7 k frames/s end to end, and giving it the chip to itself
        # between two batches' link chains costs more (77.8 k) than its 15 % buy (profiles/r03_threshold_kernels_in_the_pipeline.log;
        # at 4K 14.8 k against 15.2 k).  Detection without a link has no neighbour and takes the matrix-pipe kernel.
        # 'include luminosity in tracking calculation' (track_eval.py:290-300): every detection's mean gray value / 100 is a
        # third tracking coordinate.  Upstream offers it with 'disable gsff' only (with the filter bank its tracker raises in
        # the first update), so the tracker is built in three dimensions, in link mode 2 -- a 3-D handle of a shape the 3-D
        # batch launch serves (k_batch3: capacity <= 768, max_det about 2048) then links a batch with one launch like a 2-D
        # one, every other 3-D handle frame by frame -- and both detectors also run the luminosity kernel
        self.luminosity = bool(settings.get("include luminosity in tracking calculation", False))
        if self.luminosity and not settings["disable gsff"]:
            raise ValueError("'include luminosity in tracking calculation' needs 'disable gsff' = True")
        self.trk = DeviceTracker(max_disappeared=fps, fps=fps, n_min=settings["minimum horizon size"],
                                 n_max=settings["maximum horizon size"], n_f=settings["number of LSFFs"],
                                 use_gsff=not settings["disable gsff"], capacity=capacity, max_det=max_det,
                                 device=self.device, dimensions=3 if self.luminosity else 2,
                                 link_mode=2 if self.luminosity else 0)
        # (a handle that links a whole batch with ONE launch -- one workgroup on one compute unit -- is nobody's neighbour:
        # detection then takes the matrix-pipe kernel and its full resident grids; beside the per-frame kernels, one-launch
        # or split (4K), it keeps round 3's choice: 21.0 k against 22.3 k frames/s at 4K with the matrix-pipe kernel)
        # (... except beside the SPLIT link of large tables, where the matrix-pipe kernel on half the compute units beats both:
        # 24.3 k, profiles/r04_4k_thr_grid.log)
        beside_split_link = bool(link) and not self.trk.batched and not self.trk.fused
        beside_fused_link = bool(link) and not self.trk.batched and not beside_split_link
        #: the threshold kernel is issued on the LINK stream, between two batches' link chains, where it has the chip to
        #: itself (the labelling chain still runs beside the link, on the side stream)
        self.exclusive_threshold = False
        mode = os.environ.get("YSMR_THRESHOLD_MODE")   # (measurement aid: scripts/thr_kernels_in_pipeline.sh)
        if mode in ("beside-strip", "beside-mfma", "exclusive-mfma", "exclusive-strip"):
            beside_fused_link = mode.endswith("strip")
            self.exclusive_threshold = mode.startswith("exclusive")
        self.det = [Detector(self.B, height, width, max_det=max_det, params=params, device=self.device,
                             mean_state=mean_state, cv_flavour=settings.get("opencv version"),
                             threshold_variant=1 if beside_fused_link else 0,
                             beside_batch_link=bool(link) and self.trk.batched, beside_split_link=beside_split_link,
                             luminosity=self.luminosity)
                    for _ in range(2)]
        self.capacity = int(capacity)
        self._link = bool(link)
        n_rows = self.B * self.capacity if rows_per_flush is None else int(rows_per_flush)
        self.rows = torch.empty(n_rows * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.row_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.side = torch.cuda.Stream(device=self.device)
        self._done = [None, None]   # event: detector i's outputs consumed by the tracker
        # (events are made once and recorded again every batch: creating one costs the host tens of microseconds, and the
        # host has little slack next to a link that wants a launch every ~11 us)
        self._ev = [{k: torch.cuda.Event() for k in ("ready", "done", "thresholded")} for _ in range(2)]
        self._k = 0

    @on_own_device
    def detect_async(self, frames_dev, threshold_events=None, chain_events=None, events=None, frames_ready=None):
        """Issue detection of one batch on the side stream; returns (slot, result, ready_event).
        ``frames_ready``: what the side stream has to wait for before it reads ``frames_dev`` -- None: everything issued
        on the caller's stream so far (the frames were produced or uploaded there); an event: that event only; False:
        nothing, the frames have been resident since before the caller's stream was given its pending work (a clip in
        HBM).  The blanket wait also holds the batch back behind every link launch already issued, which drains the
        pipeline wherever one clip ends and the next begins.
        ``threshold_events``: list that receives a (start, stop) HIP event pair that the threshold kernel's own dispatch
        sets to its start and end on the device (bench.py's roofline measurement; ``Detector.threshold(timing=...)``);
        ``chain_events``: the same for the labelling / geometry chain behind it; ``events``: five ready-made timing
        events to use for these records (the first three here, the last two in ``link``) instead of new ones."""
        slot = self._k & 1
        self._k += 1
        cur = torch.cuda.current_stream(self.device)
        det = self.det[slot]
        thresholded = None
        if self.exclusive_threshold:
            e0, e1 = (events[0], events[1]) if events else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self._timed_threshold(det, frames_dev, cur, e0, e1, threshold_events is not None, bool(events))
            if threshold_events is not None:
                threshold_events.append((e0, e1, frames_dev.shape[0]))
            thresholded = self._ev[slot]["thresholded"]
            thresholded.record(cur)
        with torch.cuda.stream(self.side):
            if frames_ready is None:
                self.side.wait_stream(cur)      # the frames were produced/uploaded on the caller's stream
            elif frames_ready is not False:
                self.side.wait_event(frames_ready)
            if self._done[slot] is not None:
                self.side.wait_event(self._done[slot])
            if thresholded is not None:
                res = det.components(frames_dev.shape[0], frames=frames_dev)
                if chain_events is not None:
                    e2 = events[2] if events else torch.cuda.Event(enable_timing=True)
                    e2.record(self.side)
                    chain_events.append((e1, e2, frames_dev.shape[0]))
            elif threshold_events is None:
                res = det.detect(frames_dev)
            else:
                e0, e1 = (events[0], events[1]) if events else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self._timed_threshold(det, frames_dev, self.side, e0, e1, True, bool(events))   # (the detector's own choice of kernel)
                threshold_events.append((e0, e1, frames_dev.shape[0]))
                res = det.components(frames_dev.shape[0], frames=frames_dev)
                if chain_events is not None:
                    e2 = events[2] if events else torch.cuda.Event(enable_timing=True)
                    e2.record(self.side)
                    chain_events.append((e1, e2, frames_dev.shape[0]))
            if self._link and self.trk.batched:      # the link's binning of these detections, off the link stream
                self.trk.prepare(res.det, res.det_count, slot, third=res.lum if self.luminosity else None)
            # (with luminosity on, the calls above have also issued ysmr_luminosity_batch behind the components call, here on
            # the side stream: it reads the batch's frames, which a frame feed frees on `ready`)
            ready = self._ev[slot]["ready"]
            ready.record(self.side)
        return slot, res, ready

    @staticmethod
    def _timed_threshold(det, frames_dev, stream, e0, e1, timed, events_exist):
        """The batch's threshold launch with its duration between e0 and e1: set by the kernel's own dispatch (one
        kernel), or recorded on the stream around the call (the mean-gray branch: three kernels)."""
        if not timed:
            det.threshold(frames_dev)
        elif det.mean_state is not None:
            e0.record(stream)
            det.threshold(frames_dev)
            e1.record(stream)
        else:
            if not events_exist:
                e0.record(stream); e1.record(stream)     # (creates them; the dispatch sets them again)
            det.threshold(frames_dev, timing=(e0, e1))

    @on_own_device
    def reset(self):
        self.trk.reset()
        self.row_count.zero_()

    @on_own_device
    def link(self, slot, res, ready, first_frame, link_events=None, events=None):
        """Link one detected batch on the current stream; rows accumulate in self.rows.
        ``link_events``: list that receives a (start, stop, frames, host_seconds) record around the batch's
        launches -- HIP events on the link stream, and how long the host took to issue them."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ready)
        n = int(res.det_count.shape[0])

        def run():
            self.trk.run(res.det, res.det_count, first_frame, self.rows, self.row_count,
                         third=res.lum if self.luminosity else None)

        if link_events is None:
            run()
        else:
            e0, e1 = (events[3], events[4]) if events else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e0.record(cur)
            t0 = time.perf_counter()
            run()
            host = time.perf_counter() - t0
            e1.record(cur)
            link_events.append((e0, e1, n, host))
        done = self._ev[slot]["done"]
        done.record(cur)
        self._done[slot] = done
        return res

    def _rows_held(self):
        """Synchronise: how many rows the buffer holds (more than it has room for: an error)."""
        n = int(self.row_count.item())
        cap = self.rows.numel() // _lib.ROW_DTYPE.itemsize
        if n > cap:
            raise _lib.YsmrLibraryError(f"row buffer overflow: {n} rows > capacity {cap}")
        return n

    @on_own_device
    def take_rows(self, sort=False):
        """Synchronise, download the accumulated rows and reset the row buffer.  ``sort``: order them
        by (TRACK_ID, POSITION_T) on the device first (``sort_list``, helper_file.py:1538-1574)."""
        n = self._rows_held()
        rows = rows_to_numpy(sort_rows(self.rows, n) if sort else self.rows, n)   # (a fresh host array)
        self.row_count.zero_()
        return rows

    @on_own_device
    def take_rows_device(self):
        """Synchronise, order the accumulated rows by (TRACK_ID, POSITION_T) on the device (``sort_list``,
        helper_file.py:1538-1574), LEAVE them there and reset the row buffer: ``DeviceRows`` for ``_finish``, which prints them
        on the device too."""
        n = self._rows_held()
        out = DeviceRows(sort_rows(self.rows, n), n)
        self.row_count.zero_()
        return out

    @on_own_device
    def check(self, res):
        status = int(res.status.max().item())
        _, _, err = self.trk.info()
        if status or err:
            kind = _lib.YsmrCapacityError if (status & _lib.DET_OVERFLOW or err) else _lib.YsmrLibraryError
            raise kind(f"device path reported errors: detection status {status}, tracker {err} "
                       f"(max_det {self.det[0].max_det}, capacity {self.capacity})")


#: device-side limits when neither the call nor the settings dict name any; a video that exceeds them is
#: re-run with doubled limits (up to LIMIT_MAX), so they only decide how much HBM the first attempt takes
DEFAULT_BATCH, DEFAULT_MAX_DET, DEFAULT_CAPACITY, LIMIT_MAX = 256, 2048, 768, 32768
DEFAULT_BATCH_BYTES = 300e6


def auto_batch(height, width, channels=1):
    """Frames per batch for a video of this geometry when nobody names a number: about DEFAULT_BATCH_BYTES of frames, a
    multiple of 8 between 16 and DEFAULT_BATCH -- and, where that reaches the number of workgroups the threshold kernel
    runs on beside the one-launch batch link (``ysmr_threshold_workgroups``: 248), exactly that many: every workgroup then
    takes one whole frame and starts one item instead of two (the kernel is 5 % faster per frame)."""
    frame_bytes = max(1, int(height) * int(width) * (3 if channels == 3 else 1))
    batch = max(16, min(DEFAULT_BATCH, int(DEFAULT_BATCH_BYTES // frame_bytes) // 8 * 8))
    workgroups = int(_lib.lib().ysmr_threshold_workgroups(_lib.BESIDE_BATCH_LINK))
    return workgroups if batch >= workgroups >= 16 else batch


def track_bacteria(video_path, settings=None, result_folder=None, batch=None, max_det=None, capacity=None,
                   device="cuda:0"):
    """Detect and track bright (or dark) spots in a video; write ``<name>_list.csv``.

    Returns ``(DataFrame, fps, frame_height, frame_width, csv_path)`` or ``None`` (errors are
    logged on logger 'ysmr', never raised -- track_eval.py:50-77, 389-392, 402-404).

    ``batch`` (frames per detection launch), ``max_det`` (components per frame) and ``capacity`` (live
    tracks) size the device buffers; the reference has no such limits, so they may also be given as the
    optional settings keys 'hip frames per batch', 'hip max detections per frame', 'hip max tracks', and a
    video that overflows them is run again with both doubled (checked after the first batch and at the end).
    'include luminosity in tracking calculation' = True needs 'disable gsff' = True (with the GSFF on, the reference's own
    tracker raises in its first update: logged, ``None``); the returned table and the final csv keep their seven columns,
    as upstream's ``sort_list`` leaves them.
    Optional settings key 'hip persist rows' (default False): keep at most 'list save length interval' rows on the
    device and append every full buffer to ``<name>_list.csv`` as the reference does (helper_file.py:1403-1478), so
    that an interrupted run leaves the rows tracked so far; the file is rewritten in order at the end either way.
    Optional settings key 'hip print rows on device' (default True): the ordered rows' csv text and DataFrame columns are worked
    out on the device (``ysmr_rows_format_device``); False: on the host's threads (``ysmr_rows_write_csv_columns``) -- the same
    bytes and bits either way.  'hip stream rows' (default False): the host's threads print the rows while the video runs.
    'hip decode mjpeg' (default True): a Motion-JPEG AVI of baseline frames with restart markers is decoded on the device
    (``ysmr_mjpeg_decode_batch``); 'always': one without restart markers too -- what cameras, ffmpeg, OpenCV and Pillow write
    -- by ``ysmr_mjpeg_decode_batch_sync``, which gives such a frame a lane per 64 bytes of its entropy data instead of one in
    all; False: by Pillow on the reader threads (``frames.decode_mjpeg_setting``).
    A ``.tif`` / ``.tiff`` path is a multi-page TIFF stack, a page per frame (``frames.TiffVideo``; fps is 'frames per second', TIFF
    has none): 8-bit gray or chunky RGB strips, uncompressed, LZW (with or without the horizontal predictor) or PackBits, are
    uploaded as stored and decoded on the device (``ysmr_tiff_decode_batch``) under 'hip decode tiff' (default True; False: the
    host path -- uncompressed strips read directly, compressed ones by Pillow on the reader threads;
    ``frames.decode_tiff_setting``); other pages, and frames the device flags, are Pillow's either way.
    'hip save detection video' (default False): what upstream's window "... unfiltered possible detections" shows ('display video
    analysis', refused here) goes into ``detection_video_path(...)`` during the pass -- every frame with the boxes of its
    detections in blue and the ids and centroids of the live tracks in green (``ysmr_view_*``, csrc/view.hip); container and
    codec as ``annotate_video`` chooses them, from the same settings.  The table, the csv and the return value do not change;
    the batch is at most what ``annotate.py`` allows a pinned buffer (and the JPEG encoder's workspace) to hold.
    'hip save threshold video' (default False): what upstream's other two windows show goes into ``threshold_video_path(...)``
    in the same way (``ysmr_thrview_batch``, csrc/thrview.hip) -- True or 'mask': the window 'threshold', white where the final
    mask is set; 'markers': the window 'Adaptive double threshold markers' (only with 'adaptive double threshold' > 0: else one
    warning and no file); 'classes': the frame with kept marker pixels in red, other kept pixels in yellow and pixels that
    passed the low threshold but were dropped by the hysteresis in blue.  Any other value: a critical message and ``None``.
    """
    logger = logging.getLogger("ysmr").getChild(__name__)
    settings = get_configs(settings)
    if settings is None:
        logger.critical("No settings provided / could not get settings for track_bacteria().")
        return None
    get_loggers(log_level=settings["log_level"], logfile_name=settings["log file path"],
                short_stream_output=settings["shorten displayed logging output"],
                short_file_output=settings["shorten logfile logging output"], log_to_file=settings["log to file"])
    if not os.path.isfile(video_path):
        logger.critical("File {} does not exist".format(video_path))
        return None
    if settings["display video analysis"]:
        logger.critical("'display video analysis' = True (interactive display) is not supported by the HIP path")
        return None
    if settings["include luminosity in tracking calculation"] and not settings["disable gsff"]:
        # (ysmr/tracker.py:68-69, 222: the filter bank is built for (x, y); fed (x, y, luminosity) its first update raises
        # "ValueError: shapes (4,20) and (30,) not aligned".  The mode runs with 'disable gsff' = True, there and here.)
        logger.critical("'include luminosity in tracking calculation' = True needs 'disable gsff' = True: with the GSFF on the "
                        "reference's own tracker raises in its first update, and the HIP path has no such mode either")
        return None
    if settings["color filter"] != COLOR_BGR2GRAY:
        logger.critical("Only 'color filter = COLOR_BGR2GRAY' is supported by the HIP path")
        return None
    threshold_view = None
    if settings.get("hip save detection video") or settings.get("hip save threshold video"):
        try:      # (what 'save video file extension' / 'save video fourcc codec' / 'hip video jpeg ...' ask for, as annotate_video)
            from .annotate import output_format
            threshold_view = _threshold_view_of(settings, logger)
            if settings.get("hip save detection video") or threshold_view is not None:
                output_format(settings)
        except ValueError as exc:
            logger.critical(str(exc))
            return None
    try:
        video = open_video(video_path, default_fps=settings["frames per second"])
    except (OSError, ValueError) as exc:
        logger.exception("Cannot open file {} due to error: {}".format(video_path, exc))
        return None
    frame_count = video.frame_count
    if frame_count < settings["minimal frame count"]:
        logger.warning("File {} too short; file was skipped. Limit for 'minimal frame count': {}".format(
            video_path, settings["minimal frame count"]))
        return None
    fps_of_file = settings["frames per second"] if settings["force tracking.ini fps settings"] else video.fps
    if fps_of_file <= 0:
        logger.critical("User defined fps unacceptable: {}".format(fps_of_file))
        return None
    if not result_folder:
        result_folder = create_results_folder(video_path)
    logger.info("Starting with file {}".format(video_path))
    old_list, list_name = save_list(path=video_path, result_folder=result_folder, first_call=True,
                                    rename_old_list=settings["rename previous result .csv"])
    try:
        # The reference flips the sign of the offset IN the caller's dict for dark-on-bright videos
        # (track_eval.py:132), so a dict reused across files alternates; kept for drop-in parity.
        # threshold_params() applies the same sign change internally, from the value seen on entry.
        offset_on_entry = settings["threshold offset for detection"]
        if not settings["white bacteria on dark background"]:
            settings["threshold offset for detection"] = offset_on_entry * -1
        local = dict(settings)
        local["threshold offset for detection"] = offset_on_entry

        frame_height, frame_width = video.height, video.width
        # frames per batch when nobody names a number: ~256 MB of frames, between 16 and 256 frames (248 at 1228 x 922, 32 at 4K).
        # A batch's fixed costs -- one link launch, the detection kernels' starts, the reader's calls -- are paid per batch
        # (a 1920-frame 1228 x 922 file: 114-119 ms at 64 frames per batch, 99 ms at 256, scripts/e2e_batches.py); three pinned
        # staging buffers and two detectors' outputs of that many frames are what it costs in memory.
        batch = int(batch or settings.get("hip frames per batch") or auto_batch(frame_height, frame_width, video.channels))
        max_det = int(max_det or settings.get("hip max detections per frame") or DEFAULT_MAX_DET)
        capacity = int(capacity or settings.get("hip max tracks") or DEFAULT_CAPACITY)
        if settings.get("hip save detection video") or threshold_view is not None:
            # (a batch of a view waits in a device buffer and leaves through a pinned one: annotate.py's limits on both)
            batch = min(batch, _view_batch_limit(frame_height, frame_width, frame_count, settings))
        if threshold_view is not None:
            threshold_view = (threshold_video_path(video_path, result_folder, settings), threshold_view)
        while True:
            outcome = _device_pass(video, video_path, frame_count, fps_of_file, local, batch, max_det, capacity, device,
                                   settings, logger, list_name if settings.get("hip persist rows") else None,
                                   detection_video_path(video_path, result_folder, settings), threshold_view)
            if outcome[0] == "overflow" and 2 * max(max_det, capacity) <= LIMIT_MAX:
                max_det, capacity = 2 * max_det, max(2 * capacity, max_det)
                logger.warning("More objects than the device buffers hold in file {}: running it again with "
                               "max_det = {}, capacity = {}".format(video_path, max_det, capacity))
                continue
            if outcome[0] == "overflow":
                logger.critical("File {} holds more objects per frame than the largest device buffers ({}); "
                                "not analysed".format(video_path, LIMIT_MAX))
            break
        video.close()
        _, sorted_rows, frames_done, error_during_read, t_start, t_frames = outcome
        return _finish(video_path, settings, logger, sorted_rows, frames_done, frame_count, error_during_read, old_list,
                       list_name, fps_of_file, frame_height, frame_width, t_start, t_frames)
    finally:
        wait_for_removals()   # (a large previous list is unlinked beside the run: helper_file._remove_previous_list)


def usable_cpus():
    """CPUs this process may really use: its affinity mask, cut by the cgroup's quota (a box of this pool shows 256 CPUs and
    grants 16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fq, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fp:
                quota, period = int(fq.read()), int(fp.read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return n


class _RowDrain:
    """The tail of a video, taken off its end (39 of a 1920-frame file's 97 ms came after the last frame, all
    serial): a thread that, batch by batch, waits for the batch's link launch, brings the rows it added to the device buffer
    to the host through pinned memory on a stream of its own, and hands them to a ``RowStream`` (``ysmr_rows_stream_*``),
    whose threads print them while later batches run.  A row's text does not depend on any other row; its place in the file
    -- by (TRACK_ID, POSITION_T) -- is worked out once, at the end.  This is the frame loop's row sink under 'hip stream
    rows' (the four calls that ``_BufferedRows`` describes)."""

    def __init__(self, pipe, t_start, threads=None):
        import queue
        self.pipe, self.t_start = pipe, t_start
        self.rows_cap = pipe.rows.numel() // _lib.ROW_DTYPE.itemsize
        self.stream = RowStream(via_pandas=True, threads=threads or int(os.environ.get("YSMR_STREAM_THREADS", 0)) or max(2, min(12, usable_cpus() // 2)))
        self.copy_stream = torch.cuda.Stream(device=pipe.device)
        self.count_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.staging = torch.empty(min(self.rows_cap, pipe.B * pipe.capacity) * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8).pin_memory()
        self.taken = 0
        self.error = None
        self.q = queue.Queue()
        self.thread = threading.Thread(target=self._run, name="ysmr-row-drain", daemon=True)
        self.thread.start()

    def linked(self):
        """Behind a batch's link launch: an event of its own there (the pipeline's per-slot events are recorded again two
        batches on) for the thread to wait on."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.pipe.device))
        self.q.put(ev)

    def _run(self):
        size = _lib.ROW_DTYPE.itemsize
        with torch.cuda.device(self.pipe.device):
            while True:
                ev = self.q.get()
                try:
                    if ev is None:
                        return
                    if self.error is not None:
                        continue
                    ev.synchronize()
                    with torch.cuda.stream(self.copy_stream):
                        self.count_host.copy_(self.pipe.row_count, non_blocking=True)
                        self.copy_stream.synchronize()
                        n = int(self.count_host.item())
                        if n > self.rows_cap:
                            raise _lib.YsmrLibraryError(f"row buffer overflow: {n} rows > capacity {self.rows_cap}")
                        per = self.staging.numel() // size
                        while self.taken < n:
                            k = min(n - self.taken, per)
                            self.staging[:k * size].copy_(self.pipe.rows[self.taken * size:(self.taken + k) * size], non_blocking=True)
                            self.copy_stream.synchronize()
                            self.stream.push(self.staging.data_ptr(), k)
                            self.taken += k
                except Exception as exc:           # (kept for the caller's thread: finish() / wait_idle() raise it)
                    self.error = exc
                finally:
                    self.q.task_done()

    def make_room(self):
        """Once every batch linked so far is in the stream, the device buffer starts over."""
        self.q.join()
        if self.error is not None:
            raise self.error
        self.pipe.row_count.zero_()
        self.restart_buffer()

    def restart_buffer(self):
        self.taken = 0

    def finish(self):
        """-> the RowStream holding every row of the video (its threads may still be printing the last batch): the finished
        table, which ``_finish`` orders and writes."""
        self.q.put(None)
        self.thread.join()
        if self.error is not None:
            self.stream.close()
            raise self.error
        LAST_PASS_MARKS["last rows with the stream"] = time.perf_counter() - self.t_start
        return self.stream

    def abort(self):
        self.q.put(None)
        self.thread.join()
        self.stream.close()


_GC_LOCK = threading.Lock()
_GC_HOLDERS = 0          # frame loops of this process that currently want the heap frozen
_GC_OURS = False         # the freeze in force is this module's (not the caller's own)


def _gc_hold():
    """The first frame loop of the process freezes the collector's view of the heap, unless the caller already has
    (``gc.get_freeze_count() != 0``: that freeze is theirs and stays theirs); later loops only count themselves in."""
    global _GC_HOLDERS, _GC_OURS
    with _GC_LOCK:
        if _GC_HOLDERS == 0:
            _GC_OURS = gc.get_freeze_count() == 0
            if _GC_OURS:
                gc.freeze()
        _GC_HOLDERS += 1


def _gc_release():
    """... and only the last one to leave thaws it (two stream threads per GPU worker overlap their passes)."""
    global _GC_HOLDERS, _GC_OURS
    with _GC_LOCK:
        _GC_HOLDERS -= 1
        if _GC_HOLDERS == 0 and _GC_OURS:
            gc.unfreeze()
            _GC_OURS = False


def _persist_chunk(list_name, rows, first):
    """'hip persist rows': the rows of one full device buffer, in the order they were tracked, appended to the list
    file -- what save_list (helper_file.py:1403-1478) does every 'list save length interval' rows."""
    with open(list_name, "wb" if first else "ab") as fh:
        fh.write(rows_to_csv_bytes(rows, header=first, via_pandas=False))


class _BufferedRows:
    """The row sink of ``_device_pass`` unless 'hip stream rows' is on.  A sink is told by the frame loop to ``make_room()``
    (the next batch might not fit: the device buffer is left empty), that a batch was ``linked()``, and to ``finish()`` -> the
    video's rows as a finished table (see ``HostRows``), or to ``abort()`` an attempt that ended early.
    Here the rows stay in the device buffer and are ordered there at the end; a buffer smaller than the video goes to the
    host whenever it is full -- with ``persist_to`` ('hip persist rows') each such chunk is also appended to that list file,
    in the order the rows were tracked -- and everything is gathered and ordered in one go."""

    def __init__(self, pipe, persist_to, print_on_device):
        self.pipe, self.persist_to, self.print_on_device, self.chunks = pipe, persist_to, print_on_device, []

    def make_room(self):
        self.chunks.append(self.pipe.take_rows())
        if self.persist_to:
            _persist_chunk(self.persist_to, self.chunks[-1], len(self.chunks) == 1)

    def linked(self):
        pass

    def finish(self):
        pipe = self.pipe
        if self.chunks:      # did not fit: gather on the host, order on the device in one go
            self.chunks.append(pipe.take_rows())
            everything = np.concatenate(self.chunks)
            on_dev = torch.from_numpy(everything.view(np.uint8)).to(pipe.device)
            return HostRows(rows_to_numpy(sort_rows(on_dev, len(everything)), len(everything)))
        if self.print_on_device:
            return pipe.take_rows_device()      # (printed there too: ysmr_rows_format_device)
        return HostRows(pipe.take_rows(sort=True))

    def abort(self):      # (an attempt that ended early: its rows go nowhere)
        pass


def detection_video_path(video_path, result_folder, settings=None):
    """Where ``track_bacteria`` writes the detection view of ``video_path`` when the optional settings key 'hip save detection
    video' is on: ``<name>_detections_output.avi`` in the result folder (always an ``.avi``, uncompressed or Motion-JPEG, as
    ``annotate_video``'s file is)."""
    return os.path.join(result_folder, "{}_detections_output.avi".format(os.path.splitext(os.path.basename(video_path))[0]))


def _view_batch_limit(height, width, frame_count, settings):
    """The most frames per batch with the detection view on: what keeps one of its pinned buffers, and in Motion-JPEG mode
    the encoder's workspace, inside ``annotate.py``'s limits."""
    from . import annotate
    fmt, _, _ = annotate.output_format(settings)
    limit = annotate.auto_batch(((3 * width + 3) & ~3) * height + 8, max(frame_count, 1 << 30))
    if fmt == "mjpeg":
        limit = min(limit, annotate.DibOutput.mjpeg_batch_limit(height, width, annotate.jpeg_mode(settings)))
    return max(1, limit)


def threshold_video_path(video_path, result_folder, settings=None):
    """Where ``track_bacteria`` writes the threshold view of ``video_path`` when the optional settings key 'hip save threshold
    video' is on: ``<name>_threshold_output.avi`` in the result folder (an ``.avi``, uncompressed or Motion-JPEG, as
    ``detection_video_path``'s file is)."""
    return os.path.join(result_folder, "{}_threshold_output.avi".format(os.path.splitext(os.path.basename(video_path))[0]))


#: 'hip save threshold video' -> the ``mode`` of ysmr_thrview_batch (csrc/thrview_rule.h)
THRESHOLD_VIEW_MODES = {"mask": 0, "markers": 1, "classes": 2}


def threshold_view_mode(settings):
    """What the optional settings key 'hip save threshold video' asks for: None (absent, False, or a tracking.ini's word for
    it), else the mode of ``ysmr_thrview_batch`` -- 0 for True or 'mask', 1 for 'markers', 2 for 'classes', in any letter case;
    ValueError, naming key and value, for anything else."""
    asked = settings.get("hip save threshold video")
    if asked is None or asked is False or asked is True:
        return 0 if asked else None
    if isinstance(asked, str):
        word = asked.strip().lower()
        if word in THRESHOLD_VIEW_MODES:
            return THRESHOLD_VIEW_MODES[word]
        if word in ("true", "yes", "on", "1"):
            return 0
        if word in ("", "false", "no", "off", "0"):
            return None
    elif isinstance(asked, int) and asked == 0:
        return None
    raise ValueError("'hip save threshold video' must be True, False or one of {}, got {!r}".format(
        ", ".join(repr(k) for k in THRESHOLD_VIEW_MODES), asked))


def _threshold_view_of(settings, logger):
    """``threshold_view_mode``, and None after one warning for 'markers' where there is no marker threshold: upstream has that
    window only in the branch of 'adaptive double threshold' > 0 (ysmr/track_eval.py:189-210)."""
    mode = threshold_view_mode(settings)
    if mode == THRESHOLD_VIEW_MODES["markers"] and not settings["adaptive double threshold"] > 0:
        logger.warning("'hip save threshold video' = 'markers' needs 'adaptive double threshold' > 0 (it is {}): there are no markers, "
                       "no threshold video is written".format(settings["adaptive double threshold"]))
        return None
    return mode


class _ViewFile:
    """What the view files of ``_device_pass`` share: the file -- an ``AviWriter`` or a ``MjpegAviWriter`` on ``path``, as
    ``annotate.output_format`` reads the settings -- behind an ``annotate.DibOutput`` with a device buffer per slot, and how it
    ends.  Whatever goes wrong with the FILE (it cannot be opened, the disk is full, a write error) ends the view with a
    critical message and removes the partial file (``dead``); tracking goes on.  ``TITLE`` names the file in messages."""

    TITLE = "View video"

    def __init__(self, pipe, video, path, fps, settings, result_folder, frame_count, logger):
        from . import annotate
        self.pipe, self.path, self.logger, self.device = pipe, path, logger, pipe.device     # (device: what _on_own_device makes current)
        self.H, self.W, self.C = video.height, video.width, video.channels
        self.sink = self.writer = None
        self.dead = False
        fmt, quality, warning = annotate.output_format(settings)
        if warning:
            logger.warning("{}: {}".format(warning, path))
        try:
            os.makedirs(result_folder, exist_ok=True)
            if fmt == "mjpeg":
                mode = annotate.jpeg_mode(settings)
                self.writer = annotate.MjpegAviWriter(path, self.W, self.H, fps)
            else:
                mode = None
                if not annotate.enough_space(result_folder, annotate.AviWriter.file_bytes(self.W, self.H, frame_count), self.TITLE.lower(), logger):
                    self.dead = True
                    return
                self.writer = annotate.AviWriter(path, self.W, self.H, fps)
        except OSError as exc:         # (the file cannot be opened: no view, and tracking goes on)
            self._give_up(exc)
            return
        try:
            self.sink = annotate.DibOutput(self.writer, pipe.B, self.H, self.W, pipe.device, quality=quality, mode=mode,
                                           result_folder=result_folder, logger=logger, dib_slots=2)
            self._buffers()
        except BaseException:      # (nobody holds this object yet: the file just opened goes with it)
            self.abort()
            raise
        self.L = _lib.lib()

    def _buffers(self):
        """Device buffers of the view's own, made once the file and its ``DibOutput`` are there."""

    def _give_up(self, why):
        self.logger.critical("{} {} is not written: {}".format(self.TITLE, self.path, why))
        self.abort()

    @on_own_device
    def finish(self):
        """Everything has been painted and handed over: close the file.  -> its path, or None."""
        if self.dead:
            return None
        self.sink.close()
        if self.sink.failure:
            self._give_up(self.sink.failure[0])
            return None
        self.writer.close()
        self.dead = True
        return self.path

    @on_own_device
    def abort(self):
        """Stop, and remove what there is of the file."""
        if self.sink is not None:
            self.sink.close()
            self.sink = None
        if self.writer is not None:
            self.writer.abort()
            self.writer = None
        self.dead = True


class _ThresholdView(_ViewFile):
    """'hip save threshold video': the class map and the final mask of every batch of ``_device_pass`` as pictures
    (``ysmr_thrview_batch``, csrc/thrview.hip: the mask, the markers, or both painted over the frame), written to
    ``threshold_video_path`` during the one pass over the video.  A sibling of ``_DetectionView`` with less to wait for: a
    batch is painted into one of the two slots of its ``annotate.DibOutput`` right behind its detection, on the side
    stream, and handed over at once -- nothing here depends on the link.  Nothing here touches the detections or the rows."""

    TITLE = "Threshold video"

    def __init__(self, pipe, video, path, mode, fps, settings, result_folder, frame_count, logger):
        self.mode = int(mode)
        super().__init__(pipe, video, path, fps, settings, result_folder, frame_count, logger)

    @on_own_device
    def pack(self, frames_dev, res, first_frame):
        """Behind ``detect_async`` of a batch: its maps into a free slot, on the side stream, and out.  -> the event behind
        which the frames and the detector's maps have been read, or None."""
        if self.dead:
            return None
        try:
            k = self.sink.acquire()
        except OSError as exc:
            self._give_up(exc)
            return None
        ptr, pitch = self.sink.frames(k)
        side = self.pipe.side
        n = int(frames_dev.shape[0])
        with torch.cuda.stream(side):
            _lib.check(self.L.ysmr_thrview_batch(
                side.cuda_stream, frames_dev.data_ptr() if self.mode == 2 else None, res.cls.data_ptr(), res.mask.data_ptr(), n, self.H,
                self.W, self.C, self.mode, ptr, self.writer.stride, pitch, int(self.writer.bottom_up)), "ysmr_thrview_batch")
            packed = torch.cuda.Event()
            packed.record(side)
        if self.pipe.exclusive_threshold:
            # (that measurement mode thresholds the batch after next on the CALLER's stream, into the class map read here)
            torch.cuda.current_stream(self.device).wait_event(packed)
        try:
            if not self.sink.submit(k, n, int(first_frame), side, packed):
                self._give_up("not enough free space, {} bytes needed, {} free".format(*self.sink.shortfall))
        except OSError as exc:
            self._give_up(exc)
        return packed


class _DetectionView(_ViewFile):
    """'hip save detection video': the frames of ``_device_pass`` with every detection's box and every live track's id painted
    in (``ysmr_view_boxes_batch`` / ``ysmr_view_tracks_batch``, csrc/view.hip), written to ``detection_video_path`` during the
    one pass over the video.  The link runs a batch behind detection and a batch's frames are freed once detected, so a
    batch is packed into one of the two slots of an ``annotate.DibOutput`` right behind its detection, on the side stream,
    waits there for its link, gets its tracks on the link stream and leaves through the copy stream and the writer thread.
    Nothing here touches the detections or the rows."""

    TITLE = "Detection video"

    def __init__(self, pipe, video, path, fps, settings, result_folder, frame_count, logger):
        super().__init__(pipe, video, path, fps, settings, result_folder, frame_count, logger)
        self.row_capacity = pipe.rows.numel() // _lib.ROW_DTYPE.itemsize

    def _buffers(self):
        self.counters = torch.zeros(2, dtype=torch.int64, device=self.pipe.device)     # the row counter before / after a batch's link

    @on_own_device
    def pack(self, frames_dev, res):
        """Behind ``detect_async`` of a batch: its frames and boxes into a free slot, on the side stream.  -> (what ``tracks``
        needs, the event behind which the frames are free)."""
        if self.dead:
            return None, None
        try:
            k = self.sink.acquire()
        except OSError as exc:
            self._give_up(exc)
            return None, None
        ptr, pitch = self.sink.frames(k)
        side = self.pipe.side
        with torch.cuda.stream(side):
            _lib.check(self.L.ysmr_view_boxes_batch(
                side.cuda_stream, frames_dev.data_ptr(), int(frames_dev.shape[0]), self.H, self.W, self.C, res.det.data_ptr(),
                res.det_count.data_ptr(), self.pipe.det[0].max_det, ptr, self.writer.stride, pitch, int(self.writer.bottom_up)),
                "ysmr_view_boxes_batch")
            packed = torch.cuda.Event()
            packed.record(side)
        return (k, packed), packed

    @on_own_device
    def before_link(self):
        if not self.dead:
            self.counters[0:1].copy_(self.pipe.row_count, non_blocking=True)

    @on_own_device
    def tracks(self, held, first_frame, n):
        """Behind ``pipe.link`` of the batch, on the link stream: the rows it emitted into the packed frames, and out."""
        if self.dead or held is None:
            return
        k, packed = held
        cur = torch.cuda.current_stream(self.device)
        self.counters[1:2].copy_(self.pipe.row_count, non_blocking=True)
        cur.wait_event(packed)
        ptr, pitch = self.sink.frames(k)
        _lib.check(self.L.ysmr_view_tracks_batch(
            cur.cuda_stream, self.pipe.rows.data_ptr(), self.row_capacity, self.counters.data_ptr(), self.counters.data_ptr() + 8,
            int(first_frame), int(n), self.H, self.W, ptr, self.writer.stride, pitch, int(self.writer.bottom_up)),
            "ysmr_view_tracks_batch")
        painted = torch.cuda.Event()
        painted.record(cur)
        try:
            if not self.sink.submit(k, int(n), int(first_frame), cur, painted):
                self._give_up("not enough free space, {} bytes needed, {} free".format(*self.sink.shortfall))
        except OSError as exc:
            self._give_up(exc)


def _device_pass(video, video_path, frame_count, fps_of_file, local, batch, max_det, capacity, device, settings,
                 logger, persist_to=None, view_path=None, threshold_view=None):
    """The frame loop of one attempt.  Returns (verdict, the video's rows -- what its row sink's ``finish`` gave -- or None,
    frames done, error flag, start time, time when the last frame was linked); verdict 'overflow' asks for larger buffers."""
    frame_height, frame_width = video.height, video.width
    error_during_read = False
    frames_done = 0
    sorted_rows = None
    feed = None
    verdict = "done"
    froze = False
    sink = None
    view = None
    thr_view = None
    t_start = t_frames = time.perf_counter()
    try:
        # Rows stay on the device for the whole video when they fit (capacity rows per frame is the
        # worst case; 32 M rows = 1.3 GB) and are ordered there at the end; otherwise full buffers are
        # moved to the host in between.  ('list save length interval' bounded the reference's Python
        # list, helper_file.py:171; here it only sets the smallest buffer.)
        row_budget = min(max(frame_count, 1) * capacity, ROW_BUDGET_MAX)
        if persist_to:      # as upstream: the rows leave for the file every 'list save length interval'
            row_budget = 0
        row_budget = max(row_budget, 2 * batch * capacity, int(settings["list save length interval"]))
        pipe = TrackingPipeline(frame_height, frame_width, fps_of_file, local, batch=batch, max_det=max_det,
                                capacity=capacity, device=device, rows_per_flush=row_budget)
        LAST_PIPELINE_FACTS.clear()
        LAST_PIPELINE_FACTS.update(capacity=int(capacity), max_det=int(max_det), batched=bool(pipe.trk.batched), fused=bool(pipe.trk.fused))
        if settings.get("hip save detection video"):
            view = _DetectionView(pipe, video, view_path, fps_of_file, settings, os.path.dirname(view_path), frame_count, logger)
        if threshold_view is not None:      # (path, mode)
            thr_view = _ThresholdView(pipe, video, threshold_view[0], threshold_view[1], fps_of_file, settings,
                                      os.path.dirname(threshold_view[0]), frame_count, logger)
        pending = None
        res = None
        checked_early = False
        row_capacity = pipe.rows.numel() // _lib.ROW_DTYPE.itemsize
        rows_upper = 0     # host-side bound on the rows in the device buffer (no sync per batch)
        LAST_PASS_MARKS.clear()
        LAST_PASS_MARKS["pipeline built"] = time.perf_counter() - t_start
        feed = DeviceFrameFeed(video, pipe.B, pipe.device, decode_on_device=decode_mjpeg_setting(settings),
                               decode_tiff=decode_tiff_setting(settings))
        LAST_PASS_MARKS["feed built"] = time.perf_counter() - t_start
        # (rows leave for the host and are printed batch by batch, while later batches run -- unless they are to be appended
        # to the list file in the order they were tracked, 'hip persist rows', which is the older, serial path)
        # ('hip stream rows', default off: measured on a 16-CPU box the overlap LOSES -- 107-154 ms against the serial tail's 98 for a
        # 1920-frame file, profiles/r05_e2e_stream_threads.log: the loop's one host copy per byte of video and the printing of
        # 971 k rows are 0.43 core-seconds each, and side by side they only slow each other down)
        if persist_to is None and settings.get("hip stream rows", False):
            sink = _RowDrain(pipe, t_start)
        else:
            sink = _BufferedRows(pipe, persist_to, settings.get("hip print rows on device", True))
        # A full pass of CPython's garbage collector walks every tracked object of the process (~40 ms with torch, numpy
        # and pandas loaded) and would stall the loop that keeps the GPU fed for as long as 50 batches take; what is alive
        # now is moved out of its sight for the duration of the loop (collections of the loop's own garbage stay on).
        # (a count under a lock: with two stream threads per GPU worker the first pass to finish must not thaw the heap
        # under the other's loop)
        _gc_hold()
        froze = True
        # the link runs one batch behind detection: every turn issues a batch's detection and links the one before it, and
        # one more turn behind the feed's last batch (None) links that
        for fed in itertools.chain(feed, (None,)):
            nxt = None
            if fed is not None:
                dev, f0, n_read, feed_slot = fed
                LAST_PASS_MARKS.setdefault("first batch on the device", time.perf_counter() - t_start)
                detected = pipe.detect_async(dev)
                held, packed = view.pack(dev, detected[1]) if view is not None else (None, None)
                if thr_view is not None:       # (on the side stream too, behind the other view's: its event covers both)
                    packed = thr_view.pack(dev, detected[1], f0) or packed
                nxt = (detected, f0, n_read, held)
                feed.release(feed_slot, detected[2] if packed is None else packed)   # the batch's frames are free once its detection has run (and the view has them)
            if pending is not None:
                (slot, r, ready), p0, cnt, held = pending
                if rows_upper + cnt * pipe.capacity > row_capacity:
                    if res is not None:
                        pipe.check(res)
                    sink.make_room()
                    rows_upper = 0
                if view is not None:
                    view.before_link()
                res = pipe.link(slot, r, ready, p0)
                sink.linked()
                if view is not None:
                    view.tracks(held, p0, cnt)
                rows_upper += cnt * pipe.capacity
                frames_done = p0 + cnt
                if not checked_early:           # a video too dense for the buffers is found out after its
                    pipe.check(res)             # first batch, not after its last (one sync per video)
                    checked_early = True
            pending = nxt
        LAST_PASS_MARKS["last batch issued"] = time.perf_counter() - t_start
        if froze:
            _gc_release()
            froze = False
        if res is not None:
            torch.cuda.synchronize(pipe.device)
            t_frames = time.perf_counter()
            LAST_PASS_MARKS["last batch linked"] = t_frames - t_start
            pipe.check(res)
            if view is not None:
                written = view.finish()
                view = None
                if written:
                    logger.info("Detection video: {}".format(written))
            if thr_view is not None:
                written = thr_view.finish()
                thr_view = None
                if written:
                    logger.info("Threshold video: {}".format(written))
            sorted_rows = sink.finish()
            sink = None
        # the reference reads until cap.read() fails and accepts that only where the container said it would end, or
        # one frame earlier ("some file formats skip one frame", track_eval.py:170-174); anything else -- frames missing
        # OR frames beyond the reported count -- is its read error (:175-178)
        if frames_done not in (frame_count, frame_count - 1):
            logger.critical("Error during read with file {}".format(video_path))
            error_during_read = settings["stop evaluation on error"]
    except _lib.YsmrCapacityError as exc:
        logger.warning("{} (file {})".format(exc, video_path))
        verdict, sorted_rows, error_during_read = "overflow", None, True
    except (_lib.YsmrLibraryError, RuntimeError, ValueError) as exc:
        logger.critical("Device path failed for file {}: {}".format(video_path, exc))
        error_during_read = True
    finally:
        if froze:
            _gc_release()
        if feed is not None:
            feed.close()
        if sink is not None:        # (an attempt that ended early: its rows go nowhere)
            sink.abort()
        if view is not None:        # (... and its detection video is removed, as a failed csv is)
            view.abort()
        if thr_view is not None:
            thr_view.abort()
    return verdict, sorted_rows, frames_done, error_during_read, t_start, t_frames


def _finish(video_path, settings, logger, sorted_rows, frames_done, frame_count, error_during_read, old_list, list_name,
            fps_of_file, frame_height, frame_width, t_start, t_frames):
    """Everything after the frame loop (track_eval.py:368-405): restore the old list after an error, write
    the ordered csv, build the DataFrame."""
    if old_list and error_during_read:
        try:
            os.remove(list_name)
            os.rename(old_list, list_name)
            logger.info("Restoring old list: {}".format(list_name))
        except OSError as exc:
            logger.error("Could not restore {}: {!r}".format(list_name, exc.args))
    if sorted_rows is None or len(sorted_rows) == 0:
        if sorted_rows is not None:
            sorted_rows.close()
        logger.warning("Did not track any objects. File: {}".format(video_path))
        return None
    # track_eval.py:387-392 asks the LAST frame's tracker output for its last object id: a video whose final
    # frame has no live track (nothing seen for more than a second) "did not track any objects" upstream,
    # whatever the earlier frames held -- and the unsorted list stays on disk.  Same verdict here (the list
    # is written, ordered, before returning).
    # track_eval.py:393: sort_list(file_path=list_name, save_file=not settings['delete .csv ...']) re-reads
    # the csv with pandas, sorts it and rewrites it; the same DataFrame and the same bytes come
    # straight from the rows here (helper_file.rows_to_dataframe / rows_to_csv_bytes).
    t_rows = time.perf_counter()
    keep_file = not settings["delete .csv file after analysis"]   # (else analyse() removes the file anyway, main.py:156)
    n_rows_total = len(sorted_rows)
    try:
        try:
            _, df_for_eval = sorted_rows.finish(list_name if keep_file else None)
        except (OSError, _lib.YsmrLibraryError) as exc:
            if not keep_file:
                raise
            logger.error("Could not write {}: {}".format(list_name, exc))
            _, df_for_eval = sorted_rows.finish(None)
    finally:
        sorted_rows.close()
    alive_at_end = df_for_eval["TRACK_ID"].to_numpy()[df_for_eval["POSITION_T"].to_numpy() == frames_done - 1]
    last_id = int(alive_at_end.max()) if len(alive_at_end) else -1
    t_df = time.perf_counter()
    LAST_PASS_MARKS["csv and DataFrame done"] = t_df - t_start
    logger.debug("phases: frames {:.1f} ms, rows to host (sorted) {:.1f} ms, DataFrame {:.1f} ms, csv {:.1f} ms".format(
        (t_frames - t_start) * 1e3, (t_rows - t_frames) * 1e3, (t_df - t_rows) * 1e3, (time.perf_counter() - t_df) * 1e3))
    logger.info("objects: {}, frames: {} of {}, rows: {}, csv: {}".format(last_id + 1, frames_done, frame_count,
                                                                          n_rows_total, list_name))
    if len(alive_at_end) == 0:
        logger.warning("Did not track any objects. File: {}".format(video_path))
        return None
    if error_during_read:
        logger.critical("Error during read, stopping before evaluation. File: {}".format(video_path))
        return None
    return df_for_eval, fps_of_file, frame_height, frame_width, list_name
