"""Configuration surface and result-file helpers of the detect-and-link path.

Mirrors the parts of ``ysmr/helper_file.py`` that the hot path touches: the ``tracking.ini``
layout and the flat settings dict (``create_configs`` :143-316, ``get_configs`` :586-843), the
``*_list.csv`` wire format (``save_list`` :1403-1478, ``sort_list`` :1538-1574, ``get_data``
:846-919), ``reshape_result`` (:1336-1347) and the ``_meta.json`` side file.  Everything else in the
reference's helper module (GUI dialogs, xlsx collation, log roll-over, shutdown) belongs to the
offline/desktop half and is out of scope.
"""
from __future__ import annotations

import configparser
import json
import logging
import os
from datetime import datetime

import numpy as np

__all__ = ["create_configs", "get_configs", "default_settings", "reshape_result", "save_list", "sort_list",
           "get_data", "read_table_device", "create_results_folder", "metadata_file", "get_loggers", "COLOR_BGR2GRAY",
           "find_paths", "creation_date", "collate_results_csv_to_xlsx", "collate_xlsx_mode", "sheet_xml_host", "XLSX_MAX_ROWS",
           "LAST_COLLATE"]

COLOR_BGR2GRAY = 6  # value of cv2.COLOR_BGR2GRAY; the only colour filter the HIP path implements

#: section -> [(key, default)], same names and defaults as helper_file.py:160-284
TRACKING_INI = {
    "BASIC RECORDING SETTINGS": [
        ("pixel per micrometre", 1.41888781), ("frames per second", 30.0), ("frame height", 922),
        ("frame width", 1228), ("white bacteria on dark background", True), ("rod shaped bacteria", True),
        ("threshold offset for detection", 5)],
    "BASIC TRACK DATA ANALYSIS SETTINGS": [
        ("minimal length in seconds", 20.0), ("limit track length to x seconds", 20.0),
        ("minimal angle in degrees for turning point", 30.0), ("extreme area outliers lower end in px*px", 2),
        ("extreme area outliers upper end in px*px", 50)],
    "DISPLAY SETTINGS": [
        ("user input", True), ("select files", True), ("display video analysis", True), ("save video", False)],
    "RESULTS SETTINGS": [
        ("rename previous result .csv", False), ("delete .csv file after analysis", False),
        ("store processed .csv file", True), ("store generated statistical .csv file", True),
        ("store final analysed .csv file", True),
        ("split results by (Turn Points / Distance / Speed / Time / Displacement / perc. motile)", "perc. motile"),
        ("split violin plots on", "0.0, 20.0, 40.0, 60.0, 80.0, 100.01"), ("save large plots", True),
        ("save rose plot", True), ("save time violin plot", True), ("save acr violin plot", True),
        ("save length violin plot", True), ("save turning point violin plot", True),
        ("save speed violin plot", True), ("save angle distribution plot / bins", 36),
        ("save displacement violin plot", True), ("save percent motile plot", True),
        ("collate results csv to xlsx", True)],
    "PLOT Y-AXIS LIMITS": [
        ("turning point violin plot min", 0.0), ("turning point violin plot max", False),
        ("length violin plot min", 0.0), ("length violin plot max", False),
        ("speed violin plot min", 0.0), ("speed violin plot max", False),
        ("time violin plot min", 0.0), ("time violin plot max", False),
        ("displacement violin plot min", 0.0), ("displacement violin plot max", False),
        ("percent motile plot min", 0.0), ("percent motile plot max", 100.0),
        ("acr violin plot min", 0.0), ("acr violin plot max", 1.0)],
    "LOGGING SETTINGS": [
        ("log to file", True), ("log file path", "./logfile.log"), ("shorten displayed logging output", False),
        ("shorten logfile logging output", False), ("set logging level (debug/info/warning/critical)", "debug"),
        ("verbose", False)],
    "ADVANCED VIDEO SETTINGS": [
        ("include luminosity in tracking calculation", False), ("color filter", "COLOR_BGR2GRAY"),
        ("minimal frame count", 600), ("stop evaluation on error", True), ("list save length interval", 10000),
        ("save video file extension", ".mp4"), ("save video fourcc codec", "mp4v"),
        ("adaptive double threshold", 2.0)],
    "ADVANCED TRACK DATA ANALYSIS SETTINGS": [
        ("maximal consecutive holes", 5), ("maximal empty frames in %", 5.0),
        ("percent quantiles excluded area", 10.0), ("try to omit motility outliers", True),
        ("stop excluding motility outliers if total count above percent", 5.0),
        ("exclude measurement when above x times average area", 1.5),
        ("rod average width/height ratio min.", 0.125), ("rod average width/height ratio max.", 0.67),
        ("coccoid average width/height ratio min.", 0.8), ("coccoid average width/height ratio max.", 1.0),
        ("percent of screen edges to exclude", 5.0), ("maximal recursion depth", 960),
        ("limit track length exactly", False), ("compare angle between n frames", 10),
        ("force tracking.ini fps settings", False)],
    "GAUSSIAN-SUM FIR FILTER SETTINGS": [
        ("disable gsff", False), ("number of LSFFs", 3), ("minimum horizon size", 0),
        ("maximum horizon size", 30)],
    "HOUSEKEEPING": [("previous directory", "./"), ("shut down after analysis", False)],
    "TEST SETTINGS": [("debugging", False), ("path to test video", "Q:/test_video.avi")],
}

#: optional keys of the HIP path that a tracking.ini may carry in [ADVANCED VIDEO SETTINGS] (absent: not in the settings dict,
#: and every reader's default holds) -> how the value is read
OPTIONAL_HIP_KEYS = {"hip save detection video": "getboolean",
                     "hip save threshold video": "get"}     # (a word: track_eval.threshold_view_mode reads it)
#: ... and in [RESULTS SETTINGS], beside 'collate results csv to xlsx' (a word: collate_xlsx_mode reads it)
OPTIONAL_HIP_RESULT_KEYS = {"hip collate xlsx": "get"}

_LOG_LEVELS = {"debug": logging.DEBUG, "info": logging.INFO, "warning": logging.WARNING,
               "critical": logging.CRITICAL}


def _logger():
    return logging.getLogger("ysmr").getChild(__name__)


def create_configs(config_filepath=None):
    """(Re)write ``tracking.ini`` with the default values; an existing file is renamed with a
    timestamp first (helper_file.py:152-158).  Unlike the reference this does not try to open the
    file in a desktop editor."""
    if config_filepath is None:
        config_filepath = os.path.join(os.path.abspath("./"), "tracking.ini")
    if os.path.isfile(config_filepath):
        root, ext = os.path.splitext(config_filepath)
        os.rename(config_filepath, "{}_{}{}".format(root, datetime.now().strftime("%y%m%d%H%M%S"), ext))
    parser = configparser.ConfigParser(allow_no_value=True)
    for section, items in TRACKING_INI.items():
        parser[section] = {k: str(v) for k, v in items}
    try:
        with open(config_filepath, "w+") as fh:
            parser.write(fh)
        _logger().critical("tracking.ini was reset to default values. Path: %s", config_filepath)
    except OSError as exc:
        _logger().exception("Could not create config file: %s", exc)


def _float_or_false(text):
    try:
        return float(text)
    except (TypeError, ValueError):
        return False


def _build_settings(parser, ini_path):
    rec, trk = parser["BASIC RECORDING SETTINGS"], parser["BASIC TRACK DATA ANALYSIS SETTINGS"]
    dsp, res, yax = parser["DISPLAY SETTINGS"], parser["RESULTS SETTINGS"], parser["PLOT Y-AXIS LIMITS"]
    log, vid = parser["LOGGING SETTINGS"], parser["ADVANCED VIDEO SETTINGS"]
    adv, gsf = parser["ADVANCED TRACK DATA ANALYSIS SETTINGS"], parser["GAUSSIAN-SUM FIR FILTER SETTINGS"]
    hk, tst = parser["HOUSEKEEPING"], parser["TEST SETTINGS"]

    verbose = log.getboolean("verbose")
    level_name = log.get("set logging level (debug/info/warning/critical)")
    level = logging.DEBUG if verbose else _LOG_LEVELS.get(level_name.lower(), logging.DEBUG)
    shape = "rod" if rec.getboolean("rod shaped bacteria") else "coccoid"
    colour = vid.get("color filter")
    if colour == "COLOR_BGR2GRAY":
        colour = COLOR_BGR2GRAY
    elif colour.isdigit():
        colour = int(colour)
    splits = [float(v.strip()) for v in res.get("split violin plots on").split(",")]
    split_by = res.get("split results by (Turn Points / Distance / Speed / Time / Displacement / perc. motile)")
    warn = False
    if "perc. motile" in split_by.lower() and max(splits) == 100:
        warn = ["Violin plots are set to 'perc. motile', but 'split violin plots on' highest value is 100."]
    try:
        n_max = int(gsf.get("maximum horizon size"))
        n_max = n_max if n_max > 0 else None
    except (TypeError, ValueError):
        n_max = None

    s = {
        "pixel per micrometre": rec.getfloat("pixel per micrometre"),
        "frames per second": rec.getfloat("frames per second"),
        "frame height": rec.getint("frame height"),
        "frame width": rec.getint("frame width"),
        "white bacteria on dark background": rec.getboolean("white bacteria on dark background"),
        "rod shaped bacteria": rec.getboolean("rod shaped bacteria"),
        "threshold offset for detection": rec.getint("threshold offset for detection"),
        "minimal length in seconds": trk.getfloat("minimal length in seconds"),
        "limit track length to x seconds": trk.getfloat("limit track length to x seconds"),
        "minimal angle in degrees for turning point": trk.getfloat("minimal angle in degrees for turning point"),
        "extreme area outliers lower end in px*px": trk.getint("extreme area outliers lower end in px*px"),
        "extreme area outliers upper end in px*px": trk.getint("extreme area outliers upper end in px*px"),
        "user input": dsp.getboolean("user input"),
        "select files": dsp.getboolean("select files"),
        "display video analysis": dsp.getboolean("display video analysis"),
        "save video": dsp.getboolean("save video"),
        "split results by (Turn Points / Distance / Speed / Time / Displacement / perc. motile)": split_by,
        "split violin plots on": splits,
        "save angle distribution plot / bins": res.getint("save angle distribution plot / bins"),
    }
    for key in ("rename previous result .csv", "delete .csv file after analysis", "store processed .csv file",
                "store generated statistical .csv file", "store final analysed .csv file", "save large plots",
                "save rose plot", "save time violin plot", "save acr violin plot", "save length violin plot",
                "save turning point violin plot", "save speed violin plot", "save displacement violin plot",
                "save percent motile plot", "collate results csv to xlsx"):
        s[key] = res.getboolean(key)
    for key, _ in TRACKING_INI["PLOT Y-AXIS LIMITS"]:
        s[key] = _float_or_false(yax.get(key))
    s.update({
        "log to file": log.getboolean("log to file"),
        "log file path": log.get("log file path"),
        "shorten displayed logging output": log.getboolean("shorten displayed logging output"),
        "shorten logfile logging output": log.getboolean("shorten logfile logging output"),
        "set logging level (debug/info/warning/critical)": level_name,
        "log_level": level,
        "verbose": verbose,
        "include luminosity in tracking calculation": vid.getboolean("include luminosity in tracking calculation"),
        "color filter": colour,
        "minimal frame count": vid.getint("minimal frame count"),
        "stop evaluation on error": vid.getboolean("stop evaluation on error"),
        "list save length interval": vid.getint("list save length interval"),
        "save video file extension": vid.get("save video file extension"),
        "save video fourcc codec": vid.get("save video fourcc codec"),
        "adaptive double threshold": vid.getfloat("adaptive double threshold"),
        "maximal consecutive holes": adv.getint("maximal consecutive holes"),
        "maximal empty frames in %": adv.getfloat("maximal empty frames in %") / 100 + 1,
        "percent quantiles excluded area": adv.getfloat("percent quantiles excluded area") / 100,
        "try to omit motility outliers": adv.getboolean("try to omit motility outliers"),
        "stop excluding motility outliers if total count above percent":
            adv.getfloat("stop excluding motility outliers if total count above percent") / 100,
        "exclude measurement when above x times average area":
            adv.getfloat("exclude measurement when above x times average area"),
        "average width/height ratio min.": adv.getfloat(f"{shape} average width/height ratio min."),
        "average width/height ratio max.": adv.getfloat(f"{shape} average width/height ratio max."),
        "percent of screen edges to exclude": adv.getfloat("percent of screen edges to exclude") / 100,
        "maximal recursion depth": adv.getint("maximal recursion depth"),
        "limit track length exactly": adv.getboolean("limit track length exactly"),
        "compare angle between n frames": adv.getint("compare angle between n frames"),
        "force tracking.ini fps settings": adv.getboolean("force tracking.ini fps settings"),
        "disable gsff": gsf.getboolean("disable gsff"),
        "number of LSFFs": gsf.getint("number of LSFFs"),
        "minimum horizon size": gsf.getint("minimum horizon size"),
        "maximum horizon size": n_max,
        "previous directory": hk.get("previous directory", fallback="./"),
        "shut down after analysis": hk.getboolean("shut down after analysis"),
        "debugging": tst.getboolean("debugging"),
        "path to test video": tst.get("path to test video"),
        "tracking_ini_filepath": ini_path,
        "perc_motile_warning": warn,
    })
    for key, getter in OPTIONAL_HIP_KEYS.items():
        if vid.get(key) is not None:
            s[key] = getattr(vid, getter)(key)
    for key, getter in OPTIONAL_HIP_RESULT_KEYS.items():
        if res.get(key) is not None:
            s[key] = getattr(res, getter)(key)
    assert s["minimum horizon size"] >= 0, "'minimum horizon size' less than 0"
    assert s["number of LSFFs"] > 1, "'number of LSFFs' less than 2"
    assert s["frames per second"] > 0, "'frames per second' zero or negative"
    assert s["pixel per micrometre"] > 0 and s["frame height"] > 0 and s["frame width"] > 0
    return s


def default_settings(**overrides):
    """The settings dict ``get_configs`` would build from a pristine tracking.ini, without touching
    the file system.  The three interactive defaults (``user input``, ``select files``,
    ``display video analysis``) stay as upstream; pass overrides for headless use."""
    parser = configparser.ConfigParser(allow_no_value=True)
    for section, items in TRACKING_INI.items():
        parser[section] = {k: str(v) for k, v in items}
    s = _build_settings(parser, None)
    s.update(overrides)
    return s


def get_configs(tracking_ini_filepath=None):
    """Read ``tracking.ini`` into the flat settings dict, or pass an existing dict through
    (helper_file.py:595-596).  A missing or broken file is regenerated with defaults and ``None`` is
    returned, as upstream (helper_file.py:840-843).

    Keys that tracking.ini does not know are opt-in switches of this package, set in a settings dict and read with
    ``settings.get`` (absent: the path runs as it always has): ``'hip read csv on device'`` -- ``select_tracks`` and
    ``evaluate_tracks`` read their csv through :func:`read_table_device`, ``annotate_video`` reads an ``*_analysed.csv``
    through :func:`read_typed_device` and builds its marks on the device; ``'hip write csv on device'`` -- they write
    ``<name>_selected_data.csv`` and ``<name>_analysed.csv`` through :func:`write_table_device` (the same bytes;
    ``<name>_statistics.csv``, one row per track, stays with pandas); ``'hip png on device'`` and ``'hip violin plots'`` -- the
    figures (``evaluate.py``, ``plot_functions.py``); ``'hip collate xlsx'`` -- ``ysmr()`` ends with the collated workbook
    (:func:`collate_results_csv_to_xlsx`; the word 'deflate': compressed entries), also read from a tracking.ini's
    [RESULTS SETTINGS]."""
    if isinstance(tracking_ini_filepath, dict):
        return tracking_ini_filepath
    if tracking_ini_filepath is None:
        tracking_ini_filepath = os.path.join(os.path.abspath("./"), "tracking.ini")
    path = os.path.abspath(tracking_ini_filepath)
    parser = configparser.ConfigParser(allow_no_value=True)
    settings = None
    try:
        parser.read(path)
        settings = _build_settings(parser, path)
        missing = [k for k, v in settings.items() if v is None and k not in ("maximum horizon size",)]
        if missing:
            _logger().critical("tracking.ini is missing a value in %s", missing[0])
            settings = None
    except (TypeError, ValueError, KeyError, AssertionError, AttributeError) as exc:
        _logger().exception("An exception of type %s occurred while attempting to read tracking.ini: %r",
                            type(exc).__name__, exc.args)
    if not settings:
        create_configs(config_filepath=path)
        return None
    return settings


def get_loggers(log_level=logging.DEBUG, logfile_name="./logfile.log", short_stream_output=False,
                short_file_output=False, log_to_file=False, settings=None):
    """Attach a stream handler (and optionally a file handler) to the 'ysmr' logger once."""
    logger = logging.getLogger("ysmr")
    logger.setLevel(log_level)
    if not logger.handlers:
        fmt = "%(message)s" if short_stream_output else "{asctime} {name:25} {levelname:8} {message}"
        handler = logging.StreamHandler()
        handler.setFormatter(logging.Formatter(fmt, style="%" if short_stream_output else "{"))
        logger.addHandler(handler)
        if log_to_file and logfile_name:
            try:
                fh = logging.FileHandler(logfile_name)
                fh.setFormatter(logging.Formatter("{asctime} {name:25} {levelname:8} {message}", style="{"))
                logger.addHandler(fh)
            except OSError:
                pass
    return logger


def create_results_folder(path):
    """``<folder of path>/<yymmdd>_Results`` (created on demand)."""
    folder = os.path.join(os.path.dirname(os.path.abspath(path)), "{}_Results".format(datetime.now().strftime("%y%m%d")))
    os.makedirs(folder, exist_ok=True)
    return folder


def reshape_result(tuple_of_tuples, *args):
    """((x, y), (w, h), deg) -> ((x, y, *args), (w, h, deg))   (helper_file.py:1336-1347)."""
    (x, y), (w, h), degrees = tuple_of_tuples
    return tuple([x, y, *args]), (w, h, degrees)


CSV_HEADER = "TRACK_ID,POSITION_T,POSITION_X,POSITION_Y,WIDTH,HEIGHT,DEGREES_ANGLE\n"

# Removing a previous list of tens of megabytes is milliseconds of kernel work (its pages in the page cache are freed one by
# one: 6 ms for the 80 MB list of a 1920-frame video, as long as 150 frames take).  save_list frees the NAME at once -- the old
# file is renamed aside -- and a thread unlinks it while the video runs; track_bacteria waits for that thread before it returns.
_REMOVE_ASIDE_FROM = 8 << 20
_REMOVALS = []


def _remove_previous_list(csv_path):
    if os.path.getsize(csv_path) < _REMOVE_ASIDE_FROM:
        os.remove(csv_path)
        return
    import threading
    aside = "{}.{}.removing".format(csv_path, os.getpid())
    os.rename(csv_path, aside)

    def unlink():
        try:
            os.remove(aside)
        except OSError as exc:
            logging.getLogger("ysmr").getChild(__name__).error("Could not remove {}: {!r}".format(aside, exc.args))
    th = threading.Thread(target=unlink, name="ysmr-remove-previous-list")
    th.start()
    _REMOVALS.append(th)


def wait_for_removals():
    """Join the threads that unlink previous lists (see above)."""
    while _REMOVALS:
        _REMOVALS.pop().join()


def save_list(path, result_folder=None, coords=None, first_call=False, rename_old_list=True, illumination=False):
    """Create ``<name>_list.csv`` with its header (first_call) or append rows.

    ``coords`` items are ``(frame, id, (x, y), (w, h, deg))`` like upstream; formatting follows
    helper_file.py:1455-1475 byte for byte (``str.format`` of ints/floats).

    ``illumination`` as upstream (helper_file.py:1450-1475): the header ends in ``,ILLUMINATION`` and a row's eighth field
    is ``xy[2]`` of its ``(x, y, luminosity)``.  Deviation: ``track_bacteria`` does not go through this function -- the rows
    of a video stay on the device and ``ysmr_row`` has no third coordinate -- so with 'hip persist rows' the chunks
    appended while a luminosity run is under way keep seven columns under the seven-column header.  The final
    ``<name>_list.csv`` is the same either way: upstream's ``sort_list`` reads the eight-column file back through
    ``get_data``'s seven default columns and rewrites it with those."""
    if first_call:
        folder = result_folder if result_folder is not None else os.path.dirname(path)
        name = os.path.splitext(os.path.basename(path))[0]
        csv_path = os.path.join(folder, "{}_list.csv".format(name))
        old = False
        if os.path.isfile(csv_path):
            if rename_old_list:
                root, ext = os.path.splitext(csv_path)
                old = "{}_{}{}".format(root, datetime.now().strftime("%y%m%d%H%M%S"), ext)
                os.rename(csv_path, old)
            else:
                _remove_previous_list(csv_path)
        with open(csv_path, "w+", newline="") as fh:
            fh.write(CSV_HEADER[:-1] + ",ILLUMINATION\n" if illumination else CSV_HEADER)
        return old, csv_path
    if coords:
        lines = []
        for frame, obj_id, xy, (w, h, deg) in coords:
            line = "{0},{1},{2},{3},{4},{5},{6}".format(int(obj_id), int(frame), xy[0], xy[1], w, h, deg)
            lines.append("{},{}\n".format(line, xy[2]) if illumination else line + "\n")
        with open(path, "a", newline="") as fh:
            fh.write("".join(lines))
    return None, None


def rows_to_csv_text(rows):
    """Device rows (structured ``ysmr_row`` array) -> the text ``save_list`` would have appended.
    Disappeared tracks carry the integer zeros the reference writes (tracker.py:101, 205)."""
    out = []
    for r in rows:
        if r["disappeared"] > 0:
            w = h = deg = 0
        else:
            w, h, deg = float(r["w"]), float(r["h"]), float(r["angle"])
        out.append("{0},{1},{2},{3},{4},{5},{6}\n".format(int(r["track_id"]), int(r["frame"]), np.float64(r["x"]),
                                                          np.float64(r["y"]), w, h, deg))
    return "".join(out)


def rows_to_csv_bytes(rows, header=True, via_pandas=True, threads=0):
    """The csv the reference ends up with for these rows, as bytes: header of save_list
    (helper_file.py:1451) and one line per row formatted the way ``DataFrame.to_csv`` prints the
    uint32 / float64 columns (helper_file.py:1366-1400) -- produced by the library's native
    formatter (``ysmr_rows_format_csv``, a host function) instead of Python string formatting and
    a pandas round trip.  ``rows``: structured ``ysmr_row`` array, already in file order.
    ``via_pandas``: reproduce the 1-ulp noise of the reference's text -> read_csv detour
    (include/ysmr_hip.h); False prints the exact values."""
    return _rows_csv_buffer(rows, header, via_pandas, threads).tobytes()


def _rows_csv_buffer(rows, header, via_pandas, threads):
    import ctypes
    from . import _lib
    rows = np.ascontiguousarray(rows, dtype=_lib.ROW_DTYPE)
    L = _lib.lib()
    cap = L.ysmr_rows_csv_bound(len(rows), int(bool(header)))
    out = np.empty(cap, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    _lib.check(L.ysmr_rows_format_csv(rows.ctypes.data, len(rows), int(bool(header)), int(bool(via_pandas)), int(threads),
                                      out.ctypes.data, cap, ctypes.byref(n)), "ysmr_rows_format_csv")
    return out[:n.value]


def rows_to_csv_file(rows, path, header=True, via_pandas=True, threads=0):
    """:func:`rows_to_csv_bytes` written straight to ``path`` by the formatting threads themselves
    (``ysmr_rows_write_csv``: each writes its own piece at its place in the file)."""
    import ctypes
    from . import _lib
    rows = np.ascontiguousarray(rows, dtype=_lib.ROW_DTYPE)
    n = ctypes.c_size_t(0)
    _lib.check(_lib.lib().ysmr_rows_write_csv(rows.ctypes.data, len(rows), int(bool(header)), int(bool(via_pandas)), int(threads),
                                              os.fsencode(path), ctypes.byref(n)), "ysmr_rows_write_csv")
    return n.value


def rows_to_csv_file_and_dataframe(rows, path, header=True, via_pandas=True, threads=0):
    """``rows_to_csv_file`` and ``rows_to_dataframe`` in ONE native pass (``ysmr_rows_write_csv_columns``): the values the csv is
    printed from are the values pandas would read back from it -- worked out once for both.  Returns ``(bytes, DataFrame)``."""
    import ctypes
    import pandas as pd
    from . import _lib
    rows = np.ascontiguousarray(rows, dtype=_lib.ROW_DTYPE)
    n = len(rows)
    ids, t = np.empty(n, np.uint32), np.empty(n, np.uint32)
    cols = [np.empty(n, np.float64) for _ in range(5)]
    length = ctypes.c_size_t(0)
    _lib.check(_lib.lib().ysmr_rows_write_csv_columns(rows.ctypes.data, n, int(bool(header)), int(bool(via_pandas)), int(threads),
                                                      os.fsencode(path), ctypes.byref(length), ids.ctypes.data, t.ctypes.data,
                                                      *[c.ctypes.data for c in cols]), "ysmr_rows_write_csv_columns")
    df = pd.DataFrame({"TRACK_ID": ids, "POSITION_T": t, "POSITION_X": cols[0], "POSITION_Y": cols[1],
                       "WIDTH": cols[2], "HEIGHT": cols[3], "DEGREES_ANGLE": cols[4]})
    return length.value, df


#: pinned staging of the device formatter's results, kept between videos (pinning 100 MB costs more than the copies) -- per THREAD:
#: a GPU worker runs two stream threads whose tails may overlap
import threading as _threading
_PINNED = _threading.local()
#: (diagnostics) seconds since the call began at which the last rows_device_to_csv_file_and_dataframe reached its steps
LAST_DEVICE_ROWS_MARKS = {}


def _pinned(name, nbytes):
    import torch
    held = _PINNED.__dict__.setdefault("buffers", {})
    buf = held.get(name)
    if buf is None or buf.numel() < nbytes:
        buf = held[name] = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, pin_memory=True)
    return buf[:nbytes]


def rows_device_to_csv_file_and_dataframe(rows_u8, n, path, header=True, via_pandas=True):
    """``rows_to_csv_file_and_dataframe`` for rows that are on the DEVICE, in order (``tracker.sort_rows``): text and columns are
    worked out there (``ysmr_rows_format_device``), copied over and the text written to ``path`` (None: no file).  Returns
    ``(bytes, DataFrame)``, or ``None`` when the table holds a value the device form does not print (NaN, infinities,
    magnitudes outside 2^-20 .. 2^24): the caller then takes the host path (helper_file.py:1403-1478, 860-905, 1366-1400)."""
    import time
    import pandas as pd
    import torch
    from . import _lib
    t0 = time.perf_counter()
    marks = LAST_DEVICE_ROWS_MARKS
    marks.clear()
    L = _lib.lib()
    n = int(n)
    dev = rows_u8.device
    cap = int(L.ysmr_rows_csv_bound(n, int(bool(header))))
    ws_bytes = int(L.ysmr_rows_format_device_workspace_bytes(n)) if n else 0
    with torch.cuda.device(dev):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        csv = torch.empty(cap, dtype=torch.uint8, device=dev)
        meta = torch.zeros(2, dtype=torch.int64, device=dev)          # csv length; unserved rows (low 32 bits)
        # the seven columns in one buffer: TRACK_ID, POSITION_T (uint32), then the five float64 columns
        colbuf = torch.empty(max(n, 1) * 48, dtype=torch.uint8, device=dev)
        base = colbuf.data_ptr()
        _lib.check(L.ysmr_rows_format_device(_lib.stream_ptr(dev), rows_u8.data_ptr(), n, int(bool(header)), int(bool(via_pandas)),
                                             ws.data_ptr(), ws_bytes, csv.data_ptr(), cap, meta.data_ptr(), base, base + 4 * n,
                                             *[base + 8 * n + 8 * n * k for k in range(5)], meta[1:].data_ptr()), "ysmr_rows_format_device")
        host_cols = _pinned("columns", 48 * n)
        host_cols.copy_(colbuf[:48 * n], non_blocking=True)
        length, unserved = (int(v) for v in meta.cpu())
        marks["formatted"] = time.perf_counter() - t0
        if unserved & 0xFFFFFFFF:
            torch.cuda.current_stream(dev).synchronize()
            return None
        text = _pinned("text", length)
        text.copy_(csv[:length], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    marks["copied"] = time.perf_counter() - t0
    # the file is written by a thread of its own (the kernel's copy into the page cache: no GIL) while this one builds the table
    writer, failure = None, []
    if path is not None:
        import threading

        def write():
            try:
                _write_file(path, text.numpy())
            except OSError as exc:
                failure.append(exc)
        writer = threading.Thread(target=write)
        writer.start()
    hc = host_cols.numpy()
    ids_h, t_h = hc[:4 * n].view(np.uint32), hc[4 * n:8 * n].view(np.uint32)
    cols_h = hc[8 * n:48 * n].view(np.float64).reshape(5, n)
    # (the DataFrame copies its columns into its own blocks: the pinned staging is free for the next video)
    df = pd.DataFrame({"TRACK_ID": ids_h, "POSITION_T": t_h, "POSITION_X": cols_h[0], "POSITION_Y": cols_h[1],
                       "WIDTH": cols_h[2], "HEIGHT": cols_h[3], "DEGREES_ANGLE": cols_h[4]})
    marks["frame"] = time.perf_counter() - t0
    if writer is not None:
        writer.join()
        if failure:
            raise failure[0]
    marks["written"] = time.perf_counter() - t0
    return length, df


def _write_file(path, data):
    """``data`` (a uint8 array) to ``path`` (created or truncated).  One writer: buffered writes to ONE file take the inode's lock
    one at a time, so eight threads writing a piece each were no faster than one (60 MB: 13.5 against 14.0 ms,
    scripts/file_write_probe.py); reserving the blocks first is (11 ms)."""
    n = len(data)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
    try:
        if n >= (1 << 20):
            try:
                os.posix_fallocate(fd, 0, n)
            except OSError:
                pass                    # (a file system without it: the writes extend the file)
        view, at = memoryview(data), 0
        while at < n:
            at += os.pwrite(fd, view[at:at + (64 << 20)], at)
    except OSError:
        os.close(fd)
        fd = -1
        try:
            os.unlink(path)             # (as the native writer: no partial file is left behind)
        except OSError:
            pass
        raise
    finally:
        if fd >= 0:
            os.close(fd)


class RowStream:
    """``ysmr_rows_stream_*``: the csv and the DataFrame worked out while the video runs.  ``push`` rows (a structured
    ``_lib.ROW_DTYPE`` array, or a raw pointer and a count) as the link emits them; ``finish`` orders them by
    (TRACK_ID, POSITION_T), writes ``path`` (None: no file) and returns ``(bytes, DataFrame)`` -- what
    ``rows_to_csv_file_and_dataframe`` returns for the same rows in sorted order."""

    def __init__(self, via_pandas=True, threads=0):
        import ctypes
        from . import _lib
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().ysmr_rows_stream_create(int(threads), int(bool(via_pandas)), ctypes.byref(self._h)),
                   "ysmr_rows_stream_create")

    def push(self, rows, n=None):
        from . import _lib
        if n is None:
            rows = np.ascontiguousarray(rows, dtype=_lib.ROW_DTYPE)
            ptr, n = rows.ctypes.data, len(rows)
        else:
            ptr = int(rows)
        _lib.check(_lib.lib().ysmr_rows_stream_push(self._h, ptr, int(n)), "ysmr_rows_stream_push")

    def __len__(self):
        from . import _lib
        return int(_lib.lib().ysmr_rows_stream_count(self._h))

    def finish(self, path=None, header=True):
        import ctypes
        import pandas as pd
        from . import _lib
        n = len(self)
        ids, t = np.empty(n, np.uint32), np.empty(n, np.uint32)
        cols = [np.empty(n, np.float64) for _ in range(5)]
        length = ctypes.c_size_t(0)
        _lib.check(_lib.lib().ysmr_rows_stream_finish(self._h, int(bool(header)), None if path is None else os.fsencode(path),
                                                      ctypes.byref(length), ids.ctypes.data, t.ctypes.data,
                                                      *[c.ctypes.data for c in cols]), "ysmr_rows_stream_finish")
        df = pd.DataFrame({"TRACK_ID": ids, "POSITION_T": t, "POSITION_X": cols[0], "POSITION_Y": cols[1],
                           "WIDTH": cols[2], "HEIGHT": cols[3], "DEGREES_ANGLE": cols[4]})
        return length.value, df

    def close(self):
        from . import _lib
        if self._h:
            _lib.lib().ysmr_rows_stream_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def rows_to_dataframe(rows, via_pandas=True):
    """Rows (already sorted) -> the DataFrame ``get_data`` would have read back from the csv
    (dtypes of helper_file.py:881-889; ``via_pandas`` as in :func:`rows_to_csv_bytes`)."""
    import pandas as pd
    from . import _lib
    rows = np.ascontiguousarray(rows, dtype=_lib.ROW_DTYPE)
    n = len(rows)
    ids, t = np.empty(n, np.uint32), np.empty(n, np.uint32)
    cols = [np.empty(n, np.float64) for _ in range(5)]
    _lib.check(_lib.lib().ysmr_rows_columns(rows.ctypes.data, n, int(bool(via_pandas)), ids.ctypes.data, t.ctypes.data,
                                            *[c.ctypes.data for c in cols]), "ysmr_rows_columns")
    return pd.DataFrame({"TRACK_ID": ids, "POSITION_T": t, "POSITION_X": cols[0], "POSITION_Y": cols[1],
                         "WIDTH": cols[2], "HEIGHT": cols[3], "DEGREES_ANGLE": cols[4]})


_DTYPES = {"TRACK_ID": np.uint32, "POSITION_T": np.uint32, "POSITION_X": np.float64, "POSITION_Y": np.float64,
           "WIDTH": np.float64, "HEIGHT": np.float64, "DEGREES_ANGLE": np.float64}


def get_data(csv_file_path, dtype=None, check_sorted=True, device=None):
    """Load a ``*_list.csv`` into a DataFrame with the reference's dtypes (helper_file.py:881-889).

    ``device`` (None: pandas on the host, as ever) with the default ``dtype``: the file is read on that GPU
    (:func:`read_table_device`) -- the same DataFrame, or None, for every file."""
    import pandas as pd
    if device is not None and dtype is None:
        table = read_table_device(csv_file_path, device, check_sorted=check_sorted)
        return None if table is None else table.to_dataframe()
    dtype = _DTYPES if dtype is None else dtype
    try:
        with open(csv_file_path, "r", newline="\n") as fh:
            df = pd.read_csv(fh, sep=",", header=0, usecols=list(dtype.keys()), dtype=dtype)
    except (ValueError, OSError) as exc:
        _logger().exception(exc)
        return None
    if check_sorted and {"TRACK_ID", "POSITION_T"} <= set(dtype) and df.loc[:5, "TRACK_ID"].is_unique:
        df = sort_list(df=df, save_file=False)
    return df


def sort_list(file_path=None, sort=None, df=None, save_file=False):
    """Sort by ``TRACK_ID, POSITION_T`` (helper_file.py:1538-1574); optionally rewrite the csv."""
    sort = ["TRACK_ID", "POSITION_T"] if sort is None else ([sort] if isinstance(sort, (str, bytes)) else sort)
    if file_path is not None and df is None:
        df = get_data(file_path, check_sorted=False)
    if df is None:
        _logger().warning("No Dataframe read")
        return None
    df.sort_values(by=sort, inplace=True, na_position="first")
    df.reset_index(drop=True, inplace=True)
    if save_file and file_path is not None:
        df.to_csv(file_path, index=False)
    return df


#: (diagnostics) seconds since the call began at which the last read_table_device reached its steps
LAST_CSV_READ_MARKS = {}
#: flags of ysmr_csv_index (include/ysmr_hip.h)
CSV_FLAG_QUOTE, CSV_FLAG_CR, CSV_FLAG_NOT_PLAIN, CSV_FLAG_TOO_MANY_LINES = 1, 2, 4, 8


def csv_header_plan(line):
    """The header line of a table's csv (bytes, without its newline) -> ``(n_columns, positions)``: the position of each of
    the seven default columns, in the order of ``_DTYPES``.  None for a header the device reader does not serve: a wanted
    name missing or there twice, bytes that are not ASCII, fewer than 7 or more than 4096 names."""
    try:
        names = bytes(line).decode("ascii").split(",")
    except UnicodeDecodeError:
        return None
    if not 7 <= len(names) <= 4096 or any(names.count(k) != 1 for k in _DTYPES):
        return None
    return len(names), [names.index(k) for k in _DTYPES]


def _frame_of(columns, positions):
    """The DataFrame of seven host columns (in the order of ``_DTYPES``): pandas keeps the FILE's column order under usecols."""
    import pandas as pd
    names = list(_DTYPES)
    order = sorted(range(7), key=lambda k: positions[k])
    return pd.DataFrame({names[k]: columns[k] for k in order})


def parse_csv_devicelike(data):
    """``ysmr_csv_parse_devicelike`` on the bytes of a csv: the arithmetic of the device reader (csrc/csv_parse.h) on the host,
    for the CPU tests.  Returns ``(columns, n_rows, unserved, flags, positions)``; ``columns`` are seven arrays pre-filled
    with ones' bits (0xFFFFFFFF, a NaN), which a row that is not served leaves as they are.  None: the header is refused."""
    import ctypes
    from . import _lib
    data = bytes(data)
    end = data.find(b"\n")
    plan = csv_header_plan(data if end < 0 else data[:end])
    if plan is None or not data:
        return None
    n_columns, positions = plan
    cap = data.count(b"\n") + 1
    ids, t = np.full(cap, 0xFFFFFFFF, np.uint32), np.full(cap, 0xFFFFFFFF, np.uint32)
    cols = [np.full(cap, -1, np.int64).view(np.float64) for _ in range(5)]
    wanted = np.asarray(positions, np.int32)
    n, bad, flags = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_uint32(0)
    _lib.check(_lib.lib().ysmr_csv_parse_devicelike(data, len(data), n_columns, wanted.ctypes.data, cap, ids.ctypes.data, t.ctypes.data,
                                                    *[c.ctypes.data for c in cols], ctypes.byref(n), ctypes.byref(bad),
                                                    ctypes.byref(flags)), "ysmr_csv_parse_devicelike")
    return [a[:n.value] for a in [ids, t] + cols], n.value, bad.value, flags.value, positions


class DeviceTable:
    """What :func:`read_table_device` returns.  ``path_taken``: 'device' -- the seven columns were parsed (and ordered) on the
    GPU and are held there (``columns``: name -> tensor, the two uint32 columns as int32 bits; ``columns_dev``: the six that
    ``select_rows`` / ``evaluate_columns`` take) -- or 'host': the file is not one the device reader serves and the DataFrame
    is ``get_data``'s.  ``unserved``: rows the parse kernel counted (0 on the device path), ``flags``: of the index pass."""

    def __init__(self, path_taken, n_rows=0, columns=None, positions=None, df=None, unserved=0, flags=0, device=None, buffer=None):
        self.path_taken, self.n_rows, self.columns, self.unserved, self.flags = path_taken, n_rows, columns, unserved, flags
        self.device, self._positions, self._df, self._buffer = device, positions, df, buffer

    @property
    def columns_dev(self):
        if self.path_taken != "device" or not self.n_rows:
            return None
        return [self.columns[k] for k in list(_DTYPES)[:6]]

    def __len__(self):
        return self.n_rows

    def to_dataframe(self):
        """The DataFrame ``get_data`` returns for the file: the reference's dtypes, a RangeIndex."""
        if self._df is not None:
            return self._df
        import time
        import torch
        t0 = time.perf_counter()
        n = self.n_rows
        if n == 0:
            cols = [np.empty(0, dt) for dt in _DTYPES.values()]
        else:
            with torch.cuda.device(self.device):
                host = _pinned("columns", 48 * n)
                host.copy_(self._buffer[:48 * n], non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            hc = host.numpy()
            cols = [hc[:4 * n].view(np.uint32), hc[4 * n:8 * n].view(np.uint32)] + list(hc[8 * n:48 * n].view(np.float64).reshape(5, n))
        LAST_CSV_READ_MARKS["download"] = time.perf_counter() - t0
        # (the DataFrame copies its columns into its own blocks: the pinned staging is free for the next file)
        self._df = _frame_of(cols, self._positions)
        LAST_CSV_READ_MARKS["frame"] = time.perf_counter() - t0
        return self._df


def _split_columns(buf, n):
    import torch
    return {"TRACK_ID": buf[:4 * n].view(torch.int32), "POSITION_T": buf[4 * n:8 * n].view(torch.int32),
            **{name: buf[(8 + 8 * k) * n:(16 + 8 * k) * n].view(torch.float64) for k, name in enumerate(list(_DTYPES)[2:])}}


def read_table_device(path, device="cuda:0", check_sorted=True, sync_phases=False):
    """``get_data`` with the text-to-number work on the GPU: the file goes into a pinned buffer and up to ``device``; there
    its lines are indexed (``ysmr_csv_index``), parsed a line per lane (``ysmr_csv_parse``) and -- ``check_sorted`` and
    upstream's rough check on the first six ids -- ordered by (TRACK_ID, POSITION_T) (``ysmr_csv_order``).  Returns a
    :class:`DeviceTable`; None where ``get_data`` returns None.  A file the device reader does not serve (csrc/csv_parse.h:
    quotes, carriage returns, empty lines or fields, NaN, a header without the seven names, ...) is read by ``get_data``
    itself, exceptions and log lines included: ``path_taken == 'host'``.  ``sync_phases``: wait for the device after the
    upload and the ordering too, so that ``LAST_CSV_READ_MARKS`` tells them apart (scripts/csv_read_e2e.py)."""
    import ctypes
    import time
    import torch
    from . import _lib
    t0 = time.perf_counter()
    marks = LAST_CSV_READ_MARKS
    marks.clear()

    def host(unserved=0, flags=0):
        df = get_data(path, check_sorted=check_sorted)
        return None if df is None else DeviceTable("host", n_rows=len(df), df=df, unserved=unserved, flags=flags)

    L = _lib.lib()
    dev = torch.device(device)
    try:
        with open(path, "rb", buffering=0) as fh:
            size = os.fstat(fh.fileno()).st_size
            ws_bytes = int(L.ysmr_csv_workspace_bytes(size))
            if ws_bytes == 0:
                return host()
            staged = _pinned("csv text", size)
            view, at = memoryview(staged.numpy()), 0
            while at < size:
                got = fh.readinto(view[at:])
                if not got:
                    return host()               # (the file shrank under the read)
                at += got
    except OSError:
        return host()
    marks["file read"] = time.perf_counter() - t0
    window = 1 << 16
    while True:
        head = view[:min(window, size)].tobytes().find(b"\n")
        if head >= 0 or window >= size:
            break
        window *= 16
    plan = csv_header_plan(view[:head] if head >= 0 else view[:size])
    if plan is None:
        return host()
    n_columns, positions = plan
    wanted = np.asarray(positions, np.int32)
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        text = torch.empty((size + 255) // 256 * 256, dtype=torch.uint8, device=dev)
        text[:size].copy_(staged, non_blocking=True)
        if sync_phases:
            torch.cuda.current_stream(dev).synchronize()
            marks["upload"] = time.perf_counter() - t0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        meta = torch.zeros(4, dtype=torch.int32, device=dev)             # lines, flags, unserved
        _lib.check(L.ysmr_csv_index(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, meta.data_ptr(), meta[1:].data_ptr()),
                   "ysmr_csv_index")
        n_lines, flags = (int(v) & 0xFFFFFFFF for v in meta[:2].cpu())
        marks["index"] = time.perf_counter() - t0
        if flags:
            return host(flags=flags)
        n = n_lines - 1
        buf = torch.empty(max(48 * n, 8), dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        _lib.check(L.ysmr_csv_parse(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, n_columns, wanted.ctypes.data, n, base,
                                    base + 4 * n, *[base + 8 * n + 8 * n * k for k in range(5)], meta[2:].data_ptr()), "ysmr_csv_parse")
        # the rows not served, and the six ids of upstream's rough check (helper_file.py:892-905), in one copy
        first = min(n, 6)
        back = torch.cat([meta[2:3], buf[:4 * first].view(torch.int32)]).cpu().numpy()
        marks["parse"] = time.perf_counter() - t0
        unserved = int(back[0]) & 0xFFFFFFFF
        if unserved:
            return host(unserved=unserved)
        del text, ws
        if check_sorted and n and len(set(back[1:].tolist())) == first:
            ordered = torch.empty(48 * n, dtype=torch.uint8, device=dev)
            ows_bytes = int(L.ysmr_csv_order_workspace_bytes(n))
            ows = torch.empty(ows_bytes, dtype=torch.uint8, device=dev)
            to = ordered.data_ptr()
            _lib.check(L.ysmr_csv_order(stream, n, base, base + 4 * n, *[base + 8 * n + 8 * n * k for k in range(5)], ows.data_ptr(),
                                        ows_bytes, to, to + 4 * n, *[to + 8 * n + 8 * n * k for k in range(5)]), "ysmr_csv_order")
            buf = ordered
            if sync_phases:
                torch.cuda.current_stream(dev).synchronize()
            marks["order"] = time.perf_counter() - t0
    return DeviceTable("device", n_rows=n, columns=_split_columns(buf, n) if n else None, positions=positions, device=dev, buffer=buf)


def csv_typed_plan(header_line, names):
    """The header line of a csv (bytes, without its newline) -> ``(n_columns, positions)``: the position of each of ``names``,
    in their order.  ``csv_header_plan``'s rules for any list of names: None where a name is missing or there twice, the
    bytes are not ASCII, or the header holds more than 4096 names."""
    try:
        header = bytes(header_line).decode("ascii").split(",")
    except UnicodeDecodeError:
        return None
    names = list(names)
    if not 1 <= len(header) <= 4096 or not names or len(set(names)) != len(names) or any(header.count(k) != 1 for k in names):
        return None
    return len(header), [header.index(k) for k in names]


def _typed_fields(fields):
    """``fields``: (name, dtype) or (name, dtype, empty_is_nan) each -> [(name, numpy dtype, type code, flags)]."""
    from . import _lib
    out = []
    for field in fields:
        name, dtype = field[0], np.dtype(field[1])
        if dtype not in _lib.TABLE_COLUMN_TYPES:
            raise ValueError("column {!r}: the typed csv reader has uint32, int64, int32, int8 and float64, not {}".format(name, dtype))
        nan = len(field) > 2 and bool(field[2])
        if nan and dtype != np.float64:
            raise ValueError("column {!r}: only a float64 column reads an empty field as NaN".format(name))
        out.append((name, dtype, _lib.TABLE_COLUMN_TYPES[dtype], _lib.CSV_EMPTY_IS_NAN if nan else 0))
    if not 1 <= len(out) <= _lib.TABLE_MAX_COLUMNS:
        raise ValueError("the typed csv reader takes 1 .. {} columns, got {}".format(_lib.TABLE_MAX_COLUMNS, len(out)))
    return out


def _csv_field_array(fields, positions, pointers):
    from . import _lib
    arr = (_lib.CsvField * len(fields))()
    for k, (_name, _dtype, code, flags) in enumerate(fields):
        arr[k].data, arr[k].type, arr[k].column, arr[k].flags = pointers[k], code, positions[k], flags
    return arr


def parse_csv_typed_devicelike(data, fields):
    """``ysmr_csv_parse_typed_devicelike`` on the bytes of a csv: the arithmetic of the typed device reader (csrc/csv_parse.h)
    on the host, for the CPU tests.  ``fields``: (name, dtype[, empty_is_nan]) each.  Returns ``(columns, n_rows, unserved,
    flags)``; ``columns``: name -> array, pre-filled with ones' bits, which a row that is not served leaves as they are.
    None: the header is refused."""
    import ctypes
    from . import _lib
    data = bytes(data)
    fields = _typed_fields(fields)
    end = data.find(b"\n")
    plan = csv_typed_plan(data if end < 0 else data[:end], [f[0] for f in fields])
    if plan is None or not data:
        return None
    n_columns, positions = plan
    cap = data.count(b"\n") + 1
    cols = [np.full(cap * f[1].itemsize, 0xFF, np.uint8).view(f[1]) for f in fields]
    n, bad, flags = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_uint32(0)
    arr = _csv_field_array(fields, positions, [c.ctypes.data for c in cols])
    _lib.check(_lib.lib().ysmr_csv_parse_typed_devicelike(data, len(data), n_columns, len(fields), arr, cap, ctypes.byref(n),
                                                          ctypes.byref(bad), ctypes.byref(flags)), "ysmr_csv_parse_typed_devicelike")
    return {f[0]: c[:n.value] for f, c in zip(fields, cols)}, n.value, bad.value, flags.value


class TypedTable:
    """What :func:`read_typed_device` returns.  ``path_taken``: 'device' -- every row was parsed on the GPU and ``columns``
    (name -> tensor of ``n_rows`` values; a uint32 column as int32 bits) holds them -- or 'host': the file is not one the
    typed reader serves, nothing was read, and the caller reads it with pandas.  ``unserved``: rows the parse kernel counted
    (0 on the device path), ``flags``: of the index pass."""

    def __init__(self, path_taken, n_rows=0, columns=None, unserved=0, flags=0, device=None):
        self.path_taken, self.n_rows, self.columns, self.unserved, self.flags, self.device = path_taken, n_rows, columns, unserved, flags, device

    def __len__(self):
        return self.n_rows


def read_typed_device(path, fields, device="cuda:0", also_in_header=()):
    """The columns ``fields`` -- (name, dtype[, empty_is_nan]) each, dtype one of uint32 / int64 / int32 / int8 / float64 -- of
    the csv at ``path``, as ``pandas.read_csv(usecols, dtype)`` gives them, read on ``device``: the file goes into a pinned
    buffer and up, its lines are indexed (``ysmr_csv_index``) and parsed a line per lane (``ysmr_csv_parse_typed``).  Returns
    a :class:`TypedTable`.  What csrc/csv_parse.h does not serve -- a header without one of the names (or of
    ``also_in_header``, names that pandas' ``usecols`` would demand), quotes, carriage returns, nan / inf, an empty integer
    field, a value out of range, ... -- or a file that cannot be read gives ``path_taken == 'host'`` and no columns: the
    caller's pandas read then reports what is wrong with the file, as ever."""
    import ctypes
    import torch
    from . import _lib
    fields = _typed_fields(fields)
    L = _lib.lib()
    dev = torch.device(device)
    try:
        with open(path, "rb", buffering=0) as fh:
            size = os.fstat(fh.fileno()).st_size
            ws_bytes = int(L.ysmr_csv_workspace_bytes(size))
            if ws_bytes == 0:
                return TypedTable("host")
            staged = _pinned("csv text", size)
            view, at = memoryview(staged.numpy()), 0
            while at < size:
                got = fh.readinto(view[at:])
                if not got:
                    return TypedTable("host")           # (the file shrank under the read)
                at += got
    except OSError:
        return TypedTable("host")
    window = 1 << 16
    while True:
        head = view[:min(window, size)].tobytes().find(b"\n")
        if head >= 0 or window >= size:
            break
        window *= 16
    names = [f[0] for f in fields]
    plan = csv_typed_plan(view[:head] if head >= 0 else view[:size], names + [k for k in also_in_header if k not in names])
    if plan is None:
        return TypedTable("host")
    n_columns, positions = plan
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        text = torch.empty((size + 255) // 256 * 256, dtype=torch.uint8, device=dev)
        text[:size].copy_(staged, non_blocking=True)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        meta = torch.zeros(4, dtype=torch.int32, device=dev)             # lines, flags, unserved
        _lib.check(L.ysmr_csv_index(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, meta.data_ptr(), meta[1:].data_ptr()),
                   "ysmr_csv_index")
        n_lines, flags = (int(v) & 0xFFFFFFFF for v in meta[:2].cpu())
        if flags:
            return TypedTable("host", flags=flags)
        n = n_lines - 1
        # the columns one behind the other in one buffer, each from a 16-byte boundary
        offsets, total = [], 0
        for _name, dtype, _code, _flags in fields:
            offsets.append(total)
            total += (dtype.itemsize * n + 15) // 16 * 16
        buf = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        arr = _csv_field_array(fields, positions, [buf.data_ptr() + o for o in offsets])
        _lib.check(L.ysmr_csv_parse_typed(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, n_columns, len(fields), arr, n,
                                          meta[2:].data_ptr()), "ysmr_csv_parse_typed")
        unserved = int(meta[2:3].cpu()[0]) & 0xFFFFFFFF
        if unserved:
            return TypedTable("host", unserved=unserved)
        kinds = {np.dtype(np.uint32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
                 np.dtype(np.int8): torch.int8, np.dtype(np.float64): torch.float64}
        columns = {name: buf[o:o + dtype.itemsize * n].view(kinds[dtype]) for (name, dtype, _c, _f), o in zip(fields, offsets)}
    return TypedTable("device", n_rows=n, columns=columns, device=dev)


def _move_aside(save_path):
    """An existing ``save_path`` becomes ``<yymmddHHMMSS>.<old file name>`` beside it (helper_file.py:1366-1400)."""
    folder, name = os.path.split(save_path)
    try:
        moved = os.path.join(folder, "{}.{}".format(datetime.now().strftime("%y%m%d%H%M%S"), name))
        os.rename(save_path, moved)
        _logger().critical("Old {} renamed to {}".format(name, moved))
    except (FileNotFoundError, FileExistsError):
        pass
    except OSError as exc:
        _logger().exception("Could not move previous file {} aside: {}".format(save_path, exc))


#: (diagnostics) seconds since the call began at which the last write_table_device reached its steps
LAST_TABLE_WRITE_MARKS = {}


def table_csv_plan(df):
    """What the device writer (csrc/table_csv.hip) needs to know of a DataFrame: ``(header bytes, [numpy dtype per column])``,
    or None for a frame it does not serve -- then ``DataFrame.to_csv`` writes the whole file: no or more than 16 columns,
    column labels that are not one level of strings, a name ``to_csv`` would quote (it holds ``,``, ``"``, ``\\r`` or ``\\n``,
    or is empty) or that is not UTF-8 text, a dtype other than uint32, int64, int32, int8 and float64 (``float32`` and
    ``object`` among them)."""
    from . import _lib
    names = list(df.columns)
    if not 1 <= len(names) <= _lib.TABLE_MAX_COLUMNS or getattr(df.columns, "nlevels", 1) != 1:
        return None
    if any(not isinstance(k, str) or k == "" or any(ch in k for ch in ',"\r\n') for k in names):
        return None
    dtypes = [df.iloc[:, k].dtype for k in range(len(names))]
    if any(not isinstance(dt, np.dtype) or dt not in _lib.TABLE_COLUMN_TYPES for dt in dtypes):
        return None
    try:
        header = (",".join(names) + "\n").encode("utf-8")
    except UnicodeEncodeError:
        return None
    return header, dtypes


def _table_columns(pointers, dtypes):
    from . import _lib
    cols = (_lib.TableColumn * len(dtypes))()
    for k, (ptr, dt) in enumerate(zip(pointers, dtypes)):
        cols[k].data, cols[k].type = ptr, _lib.TABLE_COLUMN_TYPES[np.dtype(dt)]
    return cols


def _table_print_host(cap, call):
    """A printer's host twin: a buffer of the bound ``cap`` and ``call(out, cap, length, wide)`` -> ``(bytes, wide_cells)``."""
    import ctypes
    out = np.empty(max(cap, 1), np.uint8)
    length, wide = ctypes.c_size_t(0), ctypes.c_longlong(0)
    call(out.ctypes.data, cap, ctypes.byref(length), ctypes.byref(wide))
    return out[:length.value].tobytes(), wide.value


def _table_print_device(device, cap, refused, ws_bytes, launch):
    """A printer's device call: the text's buffer of the bound ``cap``, a workspace of ``ws_bytes`` and
    ``launch(stream, ws, ws_bytes, text, cap, length, wide_cells)`` with the device addresses -> ``(text, length, wide_cells)``,
    the two numbers read back with one copy; None where the sizes say the plan refuses (``refused``, or no workspace size)."""
    import torch
    from . import _lib
    if refused or ws_bytes == 0:
        return None
    with torch.cuda.device(device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        text = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
        meta = torch.zeros(2, dtype=torch.int64, device=device)          # length; wide cells (low 32 bits)
        launch(_lib.stream_ptr(device), ws.data_ptr(), ws_bytes, text.data_ptr(), cap, meta.data_ptr(), meta[1:].data_ptr())
        length, wide = (int(v) for v in meta.cpu())
    return text, length, wide & 0xFFFFFFFF


def table_csv_devicelike(df, header=None):
    """``ysmr_table_format_devicelike`` on a DataFrame: the arithmetic of the device writer (csrc/fmt.h) on the host, for the
    CPU tests.  Returns ``(bytes, wide_cells)``; None for a frame :func:`table_csv_plan` refuses.  ``header``: bytes to write
    in place of the column names' line."""
    from . import _lib
    plan = table_csv_plan(df)
    if plan is None:
        return None
    L = _lib.lib()
    head, dtypes = plan
    head = head if header is None else bytes(header)
    arrays = [np.ascontiguousarray(df.iloc[:, k].to_numpy()) for k in range(len(dtypes))]
    cols = _table_columns([a.ctypes.data for a in arrays], dtypes)
    n = len(df)
    return _table_print_host(
        int(L.ysmr_table_csv_bound(n, len(dtypes), cols, len(head))),
        lambda *where: _lib.check(L.ysmr_table_format_devicelike(n, len(dtypes), cols, head, len(head), *where), "ysmr_table_format_devicelike"))


def table_format_device(tensors, dtypes, n, header, device):
    """``ysmr_table_format_device`` on columns that are on ``device`` (``tensors``: one per column, ``n`` values of the numpy
    dtype in ``dtypes`` each, a uint32 column as its int32 bits).  Returns ``(csv, length, wide_cells)`` -- the text as a uint8
    tensor on the device, its length and the number of wide cells, read back with one copy -- or None where the plan refuses
    (more text than the 32-bit offsets hold)."""
    from . import _lib
    L = _lib.lib()
    cols = _table_columns([t.data_ptr() if n else 0 for t in tensors], dtypes)
    cap = int(L.ysmr_table_csv_bound(n, len(dtypes), cols, len(header)))
    return _table_print_device(
        device, cap, cap == 0 and bool(n or header), int(L.ysmr_table_format_workspace_bytes(n, len(dtypes), cols)),
        lambda stream, *where: _lib.check(L.ysmr_table_format_device(stream, n, len(dtypes), cols, header, len(header), *where),
                                          "ysmr_table_format_device"))


def write_table_device(df, save_path, device="cuda:0", columns_dev=None, rename_old_file=True):
    """:func:`save_df_to_csv` with the printing on the GPU (csrc/table_csv.hip): the same file, byte for byte.  The header line
    is built here, the columns that are not on ``device`` already are uploaded (``columns_dev``: name -> tensor of a column's
    values there, a uint32 column as its int32 bits; one that does not have the frame's length and item size is ignored), the
    text is printed there (``ysmr_table_format_device``), copied into a pinned buffer and written as the list's is.  The
    renaming of an older file, the log lines and the swallowing of an ``OSError`` are ``save_df_to_csv``'s; like it, the index
    is never written.  A frame the device writer does not serve (:func:`table_csv_plan`; a refusal by the plan's sizes) goes to
    ``save_df_to_csv`` unchanged, for the whole file.  Returns which path ran: ``'device'`` or ``'host'``."""
    import time
    import torch
    t0 = time.perf_counter()
    marks = LAST_TABLE_WRITE_MARKS
    marks.clear()
    plan = table_csv_plan(df)
    if plan is None:
        save_df_to_csv(df, save_path, rename_old_file=rename_old_file)
        return "host"
    header, dtypes = plan
    n = len(df)
    dev = torch.device(device)
    columns_dev = columns_dev or {}
    with torch.cuda.device(dev):
        tensors = []
        for k, (name, dt) in enumerate(zip(df.columns, dtypes)):
            held = columns_dev.get(name)
            if held is not None and held.is_cuda and held.device == dev and held.dim() == 1 and held.numel() == n and \
                    held.element_size() == dt.itemsize and held.is_contiguous() and held.dtype.is_floating_point == (dt.kind == "f"):
                tensors.append(held)
                continue
            values = np.ascontiguousarray(df.iloc[:, k].to_numpy())
            tensors.append(torch.from_numpy(values.view(np.int32) if dt == np.uint32 else values).to(dev, non_blocking=False))
        marks["upload"] = time.perf_counter() - t0
        done = table_format_device(tensors, dtypes, n, header, dev)
        if done is None:
            save_df_to_csv(df, save_path, rename_old_file=rename_old_file)
            return "host"
        csv, length, wide = done
        marks["format"] = time.perf_counter() - t0
        marks["wide cells"] = wide
        text = _pinned("table text", length)
        text.copy_(csv[:length], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    marks["download"] = time.perf_counter() - t0
    if rename_old_file:
        _move_aside(save_path)
    try:
        _write_file(save_path, text.numpy())
        _logger().debug("Selected results saved to: {}".format(save_path))
    except OSError as exc:
        _logger().exception("Could not save {}: {}".format(save_path, exc))
    marks["written"] = time.perf_counter() - t0
    return "device"


def save_df_to_csv(df, save_path, rename_old_file=True):
    """Write a DataFrame as csv without its index (helper_file.py:1366-1400); an existing file of the
    same name is first moved aside to ``<yymmddHHMMSS>.<old file name>``."""
    if rename_old_file:
        _move_aside(save_path)
    try:
        with open(save_path, "w+", newline="\n") as fh:
            df.to_csv(fh, index=False, encoding="utf-8")
        _logger().debug("Selected results saved to: {}".format(save_path))
    except OSError as exc:
        _logger().exception("Could not save {}: {}".format(save_path, exc))


def creation_date(path_to_file):
    """Seconds since the file was created -- since it was last modified where the platform keeps no creation time, as on
    Linux -- or None if there is no such file (helper_file.py:408-436)."""
    import platform
    if not os.path.isfile(path_to_file):
        return None
    if platform.system() == "Windows":
        then = os.path.getctime(path_to_file)
    else:
        stat = os.stat(path_to_file)
        then = getattr(stat, "st_birthtime", stat.st_mtime)
    return (datetime.now() - datetime.fromtimestamp(then)).total_seconds()


def find_paths(base_path, extension, minimal_age=0, maximal_age=np.inf, recursive=True):
    """The files below ``base_path`` whose names end in ``extension`` and whose age in seconds (:func:`creation_date`) lies in
    ``minimal_age .. maximal_age``, with ``/`` as separator, in glob's order; ``recursive``: sub-folders too.  A file "from the
    future" is left out with a warning unless ``minimal_age`` is negative; a path that does not exist gives None and a warning
    (helper_file.py:476-516)."""
    from glob import glob
    if not os.path.exists(base_path):
        _logger().warning("Path could not be found: {}".format(base_path))
        return None
    base_path = os.fspath(base_path)
    if base_path[-1] != "/":
        base_path += "/"
    pattern = ("{}**/*{}" if recursive else "{}*{}").format(base_path, extension)
    found = []
    for name in glob(pattern, recursive=recursive):
        name = name.replace(os.sep, "/")
        age = creation_date(name)
        if age is None:
            continue        # (a folder of that name: upstream's comparison with None raises here)
        if age < 0 and minimal_age >= 0:
            _logger().warning("The file appears to be {:.2f} seconds from the future and was thus not selected. "
                              "File: {}".format(abs(age), name))
        elif age < 0 or minimal_age <= age <= maximal_age:
            found.append(name)
    return found


# ---- the collated workbook (helper_file.py:92-137 upstream: collate_results_csv_to_xlsx) -------------------------------------
#: data rows of a sheet: Excel's 1 048 576 rows less the header's
XLSX_MAX_ROWS = 2 ** 20 - 1
#: (diagnostics) which path built each sheet of the last collate_results_csv_to_xlsx: file path -> 'device' or 'host'
LAST_COLLATE = {}
#: (diagnostics) seconds the last collate_results_csv_to_xlsx spent in each phase, summed over its files
LAST_COLLATE_TIMES = {}

_XML_HEAD = '<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n'
_NS_MAIN = "http://schemas.openxmlformats.org/spreadsheetml/2006/main"
_NS_REL = "http://schemas.openxmlformats.org/officeDocument/2006/relationships"
_NS_PKG_REL = "http://schemas.openxmlformats.org/package/2006/relationships"
_SHEET_SUFFIX = b"</sheetData></worksheet>"
#: cell formats: 0 the default; 1 bold, thin border, centred -- what pandas gives header and index cells
_STYLES_XML = (
    _XML_HEAD + '<styleSheet xmlns="' + _NS_MAIN + '">'
    '<fonts count="2"><font><sz val="11"/><name val="Calibri"/><family val="2"/></font>'
    '<font><b/><sz val="11"/><name val="Calibri"/><family val="2"/></font></fonts>'
    '<fills count="2"><fill><patternFill patternType="none"/></fill><fill><patternFill patternType="gray125"/></fill></fills>'
    '<borders count="2"><border><left/><right/><top/><bottom/><diagonal/></border>'
    '<border><left style="thin"><color auto="1"/></left><right style="thin"><color auto="1"/></right>'
    '<top style="thin"><color auto="1"/></top><bottom style="thin"><color auto="1"/></bottom><diagonal/></border></borders>'
    '<cellStyleXfs count="1"><xf numFmtId="0" fontId="0" fillId="0" borderId="0"/></cellStyleXfs>'
    '<cellXfs count="2"><xf numFmtId="0" fontId="0" fillId="0" borderId="0" xfId="0"/>'
    '<xf numFmtId="0" fontId="1" fillId="0" borderId="1" xfId="0" applyFont="1" applyBorder="1" applyAlignment="1">'
    '<alignment horizontal="center" vertical="top"/></xf></cellXfs>'
    '<cellStyles count="1"><cellStyle name="Normal" xfId="0" builtinId="0"/></cellStyles></styleSheet>')


def collate_xlsx_mode(settings):
    """What the optional settings key 'hip collate xlsx' asks for: None (absent, false, or a tracking.ini's word for false),
    'deflate' for that word in any letter case, 'stored' for every other true value."""
    asked = settings.get("hip collate xlsx")
    if isinstance(asked, str):
        word = asked.strip().lower()
        if word == "deflate":
            return "deflate"
        return None if word in ("", "false", "no", "off", "0") else "stored"
    return "stored" if asked else None


def _xml_text(text):
    """``text`` as character data or an attribute's value; what XML 1.0 cannot hold becomes Excel's ``_xHHHH_``."""
    out = str(text).replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;").replace('"', "&quot;")
    if any(ord(ch) < 32 and ch not in "\t\n\r" or ch in "\ufffe\uffff" for ch in out):
        out = "".join("_x{:04X}_".format(ord(ch)) if ord(ch) < 32 and ch not in "\t\n\r" or ch in "\ufffe\uffff" else ch for ch in out)
    return out


def _column_letters(k):
    """0 -> A, 25 -> Z, 26 -> AA, ..."""
    letters = ""
    k += 1
    while k:
        k, rest = divmod(k - 1, 26)
        letters = chr(65 + rest) + letters
    return letters


def _string_cell(ref, text, style=""):
    text = str(text)
    space = ' xml:space="preserve"' if text != text.strip() else ""
    return '<c r="{}"{} t="inlineStr"><is><t{}>{}</t></is></c>'.format(ref, style, space, _xml_text(text))


def sheet_prefix(names, header_row=1):
    """The head of a sheet's XML up to and with the header row: ``names`` in B, C, ... of row ``header_row`` as inline strings
    of style 1, column A left empty -- what ``to_excel`` writes above a frame with its RangeIndex."""
    cells = "".join(_string_cell("{}{}".format(_column_letters(k + 1), header_row), name, ' s="1"') for k, name in enumerate(names))
    return (_XML_HEAD + '<worksheet xmlns="' + _NS_MAIN + '"><sheetData><row r="{}">{}</row>'.format(header_row, cells)).encode("utf-8")


def _value_cell(ref, value):
    """One cell of the host path, '' for a missing value.  The device path's rules (csrc/xlsx_row.h) for integers and floats."""
    if value is None:
        return ""
    if isinstance(value, (bool, np.bool_)):
        return '<c r="{}" t="b"><v>{}</v></c>'.format(ref, int(value))
    if isinstance(value, (int, np.integer)):
        return '<c r="{}"><v>{}</v></c>'.format(ref, int(value))
    if isinstance(value, (float, np.floating)):
        value = float(value)
        if value != value:
            return ""
        if value in (np.inf, -np.inf):
            return _string_cell(ref, "inf" if value > 0 else "-inf")
        return '<c r="{}"><v>{}</v></c>'.format(ref, repr(value))
    try:
        import pandas as pd
        if pd.isna(value):
            return ""
    except (TypeError, ValueError):
        pass
    return _string_cell(ref, value)


def sheet_xml_host(df, first_row=2):
    """A sheet's XML for a DataFrame with a RangeIndex, in plain Python: the header row ``first_row - 1`` (:func:`sheet_prefix`),
    then a ``<row>`` per row from ``first_row`` on -- the index 0, 1, ... in column A with style 1, integers as plain decimals,
    a float64 as its shortest round-trip text (``repr``; the exact double, not ``%.16G``), a missing value not written at all,
    ``inf`` / ``-inf`` and every string as inline strings, booleans as ``t="b"``.  For a table the device path serves
    (``ysmr_xlsx_sheet_device``) these are the same bytes."""
    parts = [sheet_prefix([str(k) for k in df.columns], first_row - 1).decode("utf-8")]
    letters = [_column_letters(k + 1) for k in range(df.shape[1])]
    columns = [df.iloc[:, k].tolist() for k in range(df.shape[1])]       # (Python ints, floats, bools and objects)
    for r in range(len(df)):
        n = first_row + r
        cells = ['<c r="A{}" s="1"><v>{}</v></c>'.format(n, r)]
        cells.extend(_value_cell("{}{}".format(letters[k], n), columns[k][r]) for k in range(len(columns)))
        parts.append('<row r="{}">{}</row>'.format(n, "".join(cells)))
    parts.append(_SHEET_SUFFIX.decode("ascii"))
    return "".join(parts).encode("utf-8")


def xlsx_sheet_names(paths):
    """A sheet name per path, unique in the workbook: the file name without its extension, every character Excel forbids
    (``[ ] : * ? / \\``) as ``_``, cut to 31 characters; a name the workbook already has -- compared without regard to case,
    as Excel does -- gets its tail replaced by ``~2``, ``~3``, ... so that it still fits."""
    used, names = set(), []
    for path in paths:
        base = os.path.splitext(os.path.basename(path))[0]
        base = "".join("_" if ch in "[]:*?/\\" else ch for ch in base)[:31] or "_"
        name, k = base, 1
        while name.lower() in used:
            k += 1
            tail = "~{}".format(k)
            name = base[:31 - len(tail)] + tail
        used.add(name.lower())
        names.append(name)
    return names


def xlsx_sheet_devicelike(df, first_row=2, with_index=True, prefix=None, suffix=None):
    """``ysmr_xlsx_sheet_devicelike`` on a DataFrame of the five column types: the text of the device printer
    (csrc/xlsx_row.h) on the host, for the CPU tests.  Returns ``(bytes, wide_cells)``; None for a frame
    :func:`table_csv_plan` refuses."""
    from . import _lib
    plan = table_csv_plan(df)
    if plan is None:
        return None
    L = _lib.lib()
    dtypes = plan[1]
    prefix = sheet_prefix(list(df.columns), first_row - 1) if prefix is None else bytes(prefix)
    suffix = _SHEET_SUFFIX if suffix is None else bytes(suffix)
    arrays = [np.ascontiguousarray(df.iloc[:, k].to_numpy()) for k in range(len(dtypes))]
    cols = _table_columns([a.ctypes.data for a in arrays], dtypes)
    n = len(df)
    return _table_print_host(
        int(L.ysmr_xlsx_sheet_bound(n, len(dtypes), cols, first_row, int(with_index), len(prefix), len(suffix))),
        lambda *where: _lib.check(L.ysmr_xlsx_sheet_devicelike(n, len(dtypes), cols, first_row, int(with_index), prefix, len(prefix), suffix,
                                                               len(suffix), *where), "ysmr_xlsx_sheet_devicelike"))


def xlsx_sheet_device(tensors, dtypes, n, first_row, with_index, prefix, suffix, device):
    """``ysmr_xlsx_sheet_device`` on columns that are on ``device`` (``tensors`` as for :func:`table_format_device`).  Returns
    ``(xml, length, wide_cells)`` -- the text as a uint8 tensor on the device, its length and the number of wide cells, read
    back with one copy -- or None where the plan refuses."""
    from . import _lib
    L = _lib.lib()
    cols = _table_columns([t.data_ptr() if n else 0 for t in tensors], dtypes)
    cap = int(L.ysmr_xlsx_sheet_bound(n, len(dtypes), cols, first_row, int(with_index), len(prefix), len(suffix)))
    return _table_print_device(
        device, cap, cap == 0 and bool(n or prefix or suffix),
        int(L.ysmr_xlsx_sheet_workspace_bytes(n, len(dtypes), cols, first_row, int(with_index), len(suffix))),
        lambda stream, *where: _lib.check(L.ysmr_xlsx_sheet_device(stream, n, len(dtypes), cols, first_row, int(with_index), prefix, len(prefix),
                                                                   suffix, len(suffix), *where), "ysmr_xlsx_sheet_device"))


def csv_column_kinds_devicelike(data, n_columns):
    """``ysmr_csv_column_kinds_devicelike`` on the bytes of a csv (header line included): ``(kinds, n_rows, flags)``, ``kinds``
    a uint32 array of 17 words (``_lib.KIND_*``)."""
    import ctypes
    from . import _lib
    data = bytes(data)
    kinds = np.zeros(_lib.KIND_WORDS, np.uint32)
    n, flags = ctypes.c_longlong(0), ctypes.c_uint32(0)
    _lib.check(_lib.lib().ysmr_csv_column_kinds_devicelike(data, len(data), n_columns, kinds.ctypes.data, ctypes.byref(n), ctypes.byref(flags)),
               "ysmr_csv_column_kinds_devicelike")
    return kinds, n.value, flags.value


def column_dtypes_of_kinds(kinds, n_columns):
    """What ``pandas.read_csv`` infers for the columns whose kinds ``ysmr_csv_column_kinds`` gave: a list of ``numpy.int64`` (no
    bit set) / ``numpy.float64`` (only NOT_INT / EMPTY: NaN for the empty fields), or None -- the file goes to pandas -- where a
    line is empty or has another field count, or a column holds a field that is not a number the typed parse serves."""
    from . import _lib
    if int(kinds[_lib.KIND_WORDS - 1]):
        return None
    out = []
    for word in (int(w) for w in kinds[:n_columns]):
        if word & _lib.KIND_NOT_NUMBER:
            return None
        out.append(np.dtype(np.float64) if word else np.dtype(np.int64))
    return out


def xlsx_header_names(line):
    """The header line of a csv (bytes, without its newline) -> its names, or None where pandas would not take them as they
    stand: not UTF-8, a quote or a carriage return, more than 16 names, an empty name or one that is there twice (pandas
    renames those)."""
    from . import _lib
    try:
        names = bytes(line).decode("utf-8").split(",")
    except UnicodeDecodeError:
        return None
    if any(ch in name for name in names for ch in '"\r\x00') or not 1 <= len(names) <= _lib.TABLE_MAX_COLUMNS:
        return None
    if any(name == "" for name in names) or len(set(names)) != len(names) or names[0].startswith("\ufeff"):
        return None
    return names


def _sheet_xml_device(path, device, times):
    """The sheet of the csv at ``path`` built on ``device``: its XML in a pinned buffer (a uint8 array, valid until the next
    call of this thread) and whether rows were cut at ``XLSX_MAX_ROWS`` -- or None: the file is one for the host path."""
    import time
    import torch
    from . import _lib
    L = _lib.lib()
    dev = torch.device(device)
    clock = time.perf_counter
    t0 = clock()

    def lap(phase):
        nonlocal t0
        now = clock()
        times[phase] = times.get(phase, 0.0) + now - t0
        t0 = now
    try:
        with open(path, "rb", buffering=0) as fh:
            size = os.fstat(fh.fileno()).st_size
            ws_bytes = int(L.ysmr_csv_workspace_bytes(size))
            if ws_bytes == 0:
                return None
            staged = _pinned("csv text", size)
            view, at = memoryview(staged.numpy()), 0
            while at < size:
                got = fh.readinto(view[at:])
                if not got:
                    return None
                at += got
    except OSError:
        return None
    window = 1 << 16
    while True:
        head = view[:min(window, size)].tobytes().find(b"\n")
        if head >= 0 or window >= size:
            break
        window *= 16
    if head < 0:
        return None                                     # (a header and nothing else: pandas' empty frame)
    names = xlsx_header_names(view[:head])
    if names is None:
        return None
    # the index pass refuses a file with a byte >= 0x80 anywhere, and a statistics file has one in 'Distance (µm)': the
    # names are read, so the device gets the body behind an ASCII stand-in of the header line's length
    staged.numpy()[:head] = ord("h")
    lap("file read")
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        text = torch.empty((size + 255) // 256 * 256, dtype=torch.uint8, device=dev)
        text[:size].copy_(staged, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        lap("upload")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        meta = torch.zeros(4 + _lib.KIND_WORDS, dtype=torch.int32, device=dev)        # lines, flags, unserved, -, the kinds
        _lib.check(L.ysmr_csv_index(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, meta.data_ptr(), meta[1:].data_ptr()),
                   "ysmr_csv_index")
        n_lines, flags = (int(v) & 0xFFFFFFFF for v in meta[:2].cpu())
        if flags:
            return None
        n_all = n_lines - 1
        _lib.check(L.ysmr_csv_column_kinds(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, len(names), n_all, meta[4:].data_ptr()),
                   "ysmr_csv_column_kinds")
        kinds = meta[4:].cpu().numpy().view(np.uint32)
        lap("index + kinds")
        dtypes = column_dtypes_of_kinds(kinds, len(names))
        if dtypes is None:
            return None
        n = min(n_all, XLSX_MAX_ROWS)
        fields = [(name, dt, _lib.TABLE_COLUMN_TYPES[dt], _lib.CSV_EMPTY_IS_NAN if dt == np.float64 else 0) for name, dt in zip(names, dtypes)]
        buf = torch.empty(max(8 * n * len(fields), 16), dtype=torch.uint8, device=dev)
        pointers = [buf.data_ptr() + 8 * n * k for k in range(len(fields))]
        arr = _csv_field_array(fields, list(range(len(fields))), pointers)
        _lib.check(L.ysmr_csv_parse_typed(stream, text.data_ptr(), size, ws.data_ptr(), ws_bytes, len(names), len(fields), arr, n,
                                          meta[2:].data_ptr()), "ysmr_csv_parse_typed")
        if int(meta[2:3].cpu()[0]) & 0xFFFFFFFF:
            return None
        lap("parse")
        tensors = [buf[8 * n * k:8 * n * (k + 1)] for k in range(len(fields))]
        done = xlsx_sheet_device(tensors, dtypes, n, 2, True, sheet_prefix(names), _SHEET_SUFFIX, dev)
        if done is None:
            return None
        xml, length, _wide = done
        lap("print")
        out = _pinned("sheet xml", length)
        out.copy_(xml[:length], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        lap("download")
    return out.numpy(), n_all > n


def _sheet_xml_host_of(path):
    """The host path's sheet of the csv at ``path`` (upstream's ``read_csv`` call) and whether rows were cut."""
    import pandas as pd
    with open(path, "r", newline="\n", encoding="utf-8") as fh:
        df = pd.read_csv(fh, sep=",", header=0, encoding="utf-8")
    return sheet_xml_host(df.iloc[:XLSX_MAX_ROWS]), len(df) > XLSX_MAX_ROWS


def collate_results_csv_to_xlsx(path=None, save_path=None, csv_extension="statistics.csv", device="cuda:0", compress=False):
    """All csv files below ``path`` that end in ``csv_extension`` as the sheets of one workbook,
    ``<save_path or './'>/<yymmddHHMMSS>_collated_statistics.xlsx`` (helper_file.py:92-137), written without a third-party
    writer: a sheet per file of ``find_paths(path, csv_extension)``, in that order, named by :func:`xlsx_sheet_names`; row 1
    the column names, column A the RangeIndex, at most ``XLSX_MAX_ROWS`` data rows (one warning per file cut).  A file the
    device reader serves -- comma separated columns that ``pandas.read_csv`` infers as int64 or float64, up to 16 of them,
    distinct names, no quotes or carriage returns -- is read, typed and printed on ``device`` (``ysmr_csv_column_kinds``,
    ``ysmr_csv_parse_typed``, ``ysmr_xlsx_sheet_device``); every other file is read by pandas and printed by
    :func:`sheet_xml_host`: the same bytes where both serve a file.  ``device=None``: the host path for every file.
    ``LAST_COLLATE`` says which path each file took.  The container is ``zipfile``'s, stored or (``compress``) deflated, every
    entry dated 1980-01-01: the same input gives the same workbook.  Returns the workbook's path; None -- nothing written --
    where ``path`` is None (no file dialog here) or holds no such file."""
    import time
    import zipfile
    logger = _logger()
    LAST_COLLATE.clear()
    LAST_COLLATE_TIMES.clear()
    if path is None:
        logger.critical("collate_results_csv_to_xlsx needs the folder with the csv files ('path': there is no file dialog here).")
        return None
    if save_path is None:
        save_path = "./"
    file_path = os.path.join(save_path, "{}_collated_statistics.xlsx".format(datetime.now().strftime("%y%m%d%H%M%S")))
    paths = find_paths(base_path=path, extension=csv_extension)
    if not paths:
        logger.warning("Could not find paths.")
        return None
    names = xlsx_sheet_names(paths)
    times = LAST_COLLATE_TIMES
    method = zipfile.ZIP_DEFLATED if compress else zipfile.ZIP_STORED

    def entry(archive, name, data):
        info = zipfile.ZipInfo(name, date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = method
        t0 = time.perf_counter()
        archive.writestr(info, data)
        times["zip"] = times.get("zip", 0.0) + time.perf_counter() - t0

    count = len(paths)

    def write(archive):
        entry(archive, "[Content_Types].xml", _XML_HEAD + (
            '<Types xmlns="http://schemas.openxmlformats.org/package/2006/content-types">'
            '<Default Extension="rels" ContentType="application/vnd.openxmlformats-package.relationships+xml"/>'
            '<Default Extension="xml" ContentType="application/xml"/>'
            '<Override PartName="/xl/workbook.xml" ContentType="application/vnd.openxmlformats-officedocument.spreadsheetml.sheet.main+xml"/>'
            '<Override PartName="/xl/styles.xml" ContentType="application/vnd.openxmlformats-officedocument.spreadsheetml.styles+xml"/>'
            + "".join('<Override PartName="/xl/worksheets/sheet{}.xml" ContentType="application/vnd.openxmlformats-officedocument.'
                      'spreadsheetml.worksheet+xml"/>'.format(k + 1) for k in range(count)) + "</Types>"))
        entry(archive, "_rels/.rels", _XML_HEAD + (
            '<Relationships xmlns="' + _NS_PKG_REL + '"><Relationship Id="rId1" Type="' + _NS_REL + '/officeDocument" '
            'Target="xl/workbook.xml"/></Relationships>'))
        entry(archive, "xl/workbook.xml", _XML_HEAD + (
            '<workbook xmlns="' + _NS_MAIN + '" xmlns:r="' + _NS_REL + '"><sheets>'
            + "".join('<sheet name="{}" sheetId="{}" r:id="rId{}"/>'.format(_xml_text(name), k + 1, k + 1) for k, name in enumerate(names))
            + "</sheets></workbook>"))
        entry(archive, "xl/_rels/workbook.xml.rels", _XML_HEAD + (
            '<Relationships xmlns="' + _NS_PKG_REL + '">'
            + "".join('<Relationship Id="rId{}" Type="{}/worksheet" Target="worksheets/sheet{}.xml"/>'.format(k + 1, _NS_REL, k + 1)
                      for k in range(count))
            + '<Relationship Id="rId{}" Type="{}/styles" Target="styles.xml"/></Relationships>'.format(count + 1, _NS_REL)))
        entry(archive, "xl/styles.xml", _STYLES_XML)
        for k, csv_path in enumerate(paths):
            done = _sheet_xml_device(csv_path, device, times) if device is not None else None
            LAST_COLLATE[csv_path] = "device" if done is not None else "host"
            if done is None:
                t0 = time.perf_counter()
                done = _sheet_xml_host_of(csv_path)
                times["host sheet"] = times.get("host sheet", 0.0) + time.perf_counter() - t0
            xml, cut = done
            if cut:
                logger.warning("{}: more than {} rows, the sheet holds the first {}.".format(csv_path, XLSX_MAX_ROWS, XLSX_MAX_ROWS))
            entry(archive, "xl/worksheets/sheet{}.xml".format(k + 1), memoryview(xml))
    try:
        with zipfile.ZipFile(file_path, "w", method) as archive:
            write(archive)
    except BaseException:
        try:                                 # (half a workbook is none: a reader would take it for the run's result)
            os.remove(file_path)
        except OSError:
            pass
        raise
    logger.info("Collated {} file(s) into {}".format(count, file_path))
    return file_path


def _meta_path_of(path):
    """``<name>_meta.json`` for a video, one of the pipeline's own csv files, or a meta file itself."""
    path = os.fspath(path)
    if path.endswith("_meta.json"):
        return path
    for ext in ("_analysed.csv", "_list.csv", "_selected_data.csv", "_statistics.csv"):
        if path.endswith(ext):
            return path[: -len(ext)] + "_meta.json"
    return os.path.splitext(path)[0] + "_meta.json"


def metadata_file(path=None, verbose=False, additional_search_paths=None, **kwargs):
    """Read/update the ``<name>_meta.json`` side file (fps, frame_height, frame_width, caller's notes).
    Looked for next to ``path``, in the folder above it, then next to every additional search path; the
    first one found is read and, when new non-None values are given, rewritten in place (none found: it is
    created next to ``path``).  New values win over stored ones (helper_file.py:1267-1333)."""
    path = os.fspath(path)
    folder, name = os.path.split(path)
    candidates = [path, os.path.join(os.path.dirname(folder), name)]
    if additional_search_paths:
        if isinstance(additional_search_paths, (str, os.PathLike)):
            candidates.append(additional_search_paths)
        else:
            candidates.extend(additional_search_paths)
    candidates = [_meta_path_of(c) for c in candidates]
    meta, meta_path = {}, candidates[0]
    for cand in candidates:
        if verbose:
            _logger().debug("Searching for meta file in path: {}".format(cand))
        try:
            with open(cand) as fh:
                stored = json.load(fh)
        except (OSError, ValueError):
            continue
        meta.update({k: v for k, v in stored.items() if v is not None})
        meta_path = cand
        break
    new = {k: v for k, v in kwargs.items() if v is not None}
    if new:
        meta.update(new)
        try:
            with open(meta_path, "w+") as fh:
                json.dump(meta, fh)
        except OSError as exc:
            _logger().exception(exc)
    return meta
