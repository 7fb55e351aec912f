"""``evaluate_tracks`` -- per-track statistics of the selected tracks on the device.

Host mirror of the reference's function (ysmr/track_eval.py:846-1318): same signature, same argument checks and
log lines, same result files (``<name>_statistics.csv``, ``<name>_analysed.csv``, written with the reference's own
``DataFrame.to_csv`` call) and the same return value ``(df, df_stats)``.  Everything numerical happens in
``ysmr_evaluate_tracks`` (``csrc/evaluate.hip``).  The overview, the rose graph and the angle histogram are painted
on the device (``plot_functions``, ``csrc/plots.hip``) under the reference's settings and file names.  The violin
plots (seaborn figures upstream) are drawn by ``plot_functions.violin_plot`` (``csrc/violin.hip``) when the settings
hold a true 'hip violin plots'; without that key the settings that ask for them are noted in the log and skipped.
"""
from __future__ import annotations

import ctypes
import logging
import os

import numpy as np

from . import _lib
from .helper_file import create_results_folder, get_configs, get_data, read_table_device, save_df_to_csv, write_table_device

__all__ = ["evaluate_tracks", "evaluate_params", "evaluate_columns"]

STATS_COLUMNS = ["Turn Points (TP/s)", "Distance (µm)", "Speed (µm/s)", "Time (s)", "Displacement (µm)",
                 "Perc. Motile", "Arc-Chord Ratio", "Bacteria Length", "Displacement divided by length",
                 "Motility Phenotype", "TRACK_ID", "Median Speed"]
ROW_COLUMNS = ["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE", "angle_diff",
               "moving", "turn_points", "tp_of_tracks", "travelled_dist", "motility_phenotype"]
#: figures drawn only under 'hip violin plots'
_SKIPPED_PLOT_KEYS = ("save time violin plot", "save acr violin plot", "save length violin plot",
                      "save turning point violin plot", "save speed violin plot", "save displacement violin plot",
                      "save percent motile plot")


#: upstream's violin figures in its order (track_eval.py:1237-1290): settings key, column, file name, keys of the y limits
VIOLIN_FIGURES = (("save turning point violin plot", 0, "turning_points", "turning point violin plot"),
                  ("save length violin plot", 1, "distance", "length violin plot"),
                  ("save speed violin plot", 2, "speed", "speed violin plot"),
                  ("save time violin plot", 3, "time_plot", "time violin plot"),
                  ("save displacement violin plot", 4, "displacement", "displacement violin plot"),
                  ("save percent motile plot", 5, "perc_motile", "percent motile plot"),
                  ("save acr violin plot", 6, "arc-chord_ratio", "acr violin plot"))


def violin_cut_list(parameter, splits):
    """The (low, high, name) triples of the violins (track_eval.py:1164-1179): 'All' in front, then the consecutive pairs
    of 'split violin plots on' -- or the three phenotypes when the tracks are split by 'Motility Phenotype'."""
    if parameter == STATS_COLUMNS[5]:
        cuts = [(a, b, "{:.1f}% - {:.1f}%".format(a, b)) for a, b in zip(splits[:-1], splits[1:])]
    elif parameter == STATS_COLUMNS[9]:
        cuts = [(0, 0.001, "Immotile"), (1, 1.001, "Twitching"), (2, 2.001, "Motile")]
    else:
        cuts = [(a, b, "{:.2f} - {:.2f}".format(a, b)) for a, b in zip(splits[:-1], splits[1:])]
    return [(-np.inf, np.inf, "All")] + cuts


def plot_title(file_name):
    """The figures' title (track_eval.py:882-895): the file name with spaces for underscores, without a trailing
    '_selected_data', and twelve leading digits read as a date (yymmddHHMMSS)."""
    from time import strftime, strptime
    title = file_name.replace("_", " ")
    if "_selected_data" in file_name:
        title = title[:-len("_selected_data")]
    stamp = title[:12]
    if len(stamp) == 12 and stamp.isdigit():
        try:
            title = "{} {}".format(strftime("%d. %m. '%y,", strptime(stamp, "%y%m%d%H%M%S")), title[12:])
        except ValueError:
            pass
    return title


def _figures(out, stats, settings, title, save_path, device, logger, df_stats=None, parameter=None):
    """The figures where the reference draws them (track_eval.py:950-957, 1216-1303).  A figure that fails is an
    error in the log; the tables and the csv files do not depend on it."""
    from . import plot_functions as pf
    px = settings["pixel per micrometre"]
    # lettering and deflate in csrc/png.hip: absent or false -- the host path; 'dynamic' (any case) -- the dynamic stream,
    # the smaller files; anything else true -- the fixed code
    on_device = {None: False, "fixed": True, "dynamic": "dynamic"}[pf.png_mode(settings.get("hip png on device"))]
    jobs = []
    if settings.get("save angle distribution plot / bins"):
        jobs.append(("angle_histogram", lambda path: pf.angle_distribution_plot(
            df=out, bins_number=settings["save angle distribution plot / bins"], plot_title_name=title, save_path=path,
            compare_n_frames=settings["compare angle between n frames"], device=device, png_on_device=on_device)))
    distances = np.ascontiguousarray(stats[:, 1])
    span = dict(dist_min=float(distances.min()), dist_max=float(distances.max())) if len(distances) else {}
    if settings.get("save large plots"):
        jobs.append(("Bac_Run_Overview", lambda path: pf.large_xy_plot(
            df=out, plot_title_name=title, save_path=path, px_to_micrometre=px, distances=distances, device=device, png_on_device=on_device, **span)))
    if settings.get("save rose plot"):
        jobs.append(("rose_graph", lambda path: pf.rose_graph(
            df=out, plot_title_name=title, save_path=path, px_to_micrometre=px, distances=distances, device=device, png_on_device=on_device, **span)))
    if settings.get("hip violin plots") and df_stats is not None:
        cut_list = violin_cut_list(parameter, settings["split violin plots on"])
        chosen = [(STATS_COLUMNS[col], name, settings.get(limits + " min"), settings.get(limits + " max"))
                  for key, col, name, limits in VIOLIN_FIGURES if settings.get(key)]
        chosen.append((STATS_COLUMNS[11], "Median_speed", None, None))
        for column, name, y_min, y_max in chosen:
            jobs.append((name, lambda path, column=column, y_min=y_min, y_max=y_max: pf.violin_plot(
                df=df_stats, save_path=path, category=column, cut_off_category="Categories ({})".format(parameter),
                cut_off_list=cut_list, plot_title_name=title, y_min=y_min, y_max=y_max, device=device, png_on_device=on_device)))
    for name, job in jobs:
        try:
            job(save_path.format(name, ".png"))
        except Exception as exc:   # noqa: BLE001 -- whatever went wrong in a figure, the results stand
            logger.error("Figure {} failed: {}".format(save_path.format(name, ".png"), exc))


def evaluate_params(settings, fps) -> _lib.EvaluateParams:
    """The scalars ``ysmr_evaluate_tracks`` needs (track_eval.py:931-934, 941, 957, 990-1000)."""
    p = _lib.EvaluateParams()
    p.pixel_per_micrometre = float(settings["pixel per micrometre"])
    p.fps = float(fps)
    p.min_turn_angle = float(settings["minimal angle in degrees for turning point"])
    p.angle_lag = int(settings["compare angle between n frames"])
    spans = [10] + [v / 2 for v in (settings["minimal length in seconds"], settings["limit track length to x seconds"])
                    if 0 < v / 2 < 10]
    p.reach_lag = int(round(fps * min(spans), 0))
    second = int(round(fps, 0))
    p.median_kernel = second + 1 if second % 2 == 0 else second
    return p


def evaluate_columns(df, params: _lib.EvaluateParams, device="cuda:0", columns_dev=None, keep_device=False):
    """Run ``ysmr_evaluate_tracks`` on the table's six input columns.  Returns (dict of per-row arrays,
    statistics array [tracks, 12]).  ``columns_dev``: those six columns where they are on ``device`` already
    (``DeviceTable.columns_dev`` of ``helper_file.read_table_device``): nothing is uploaded.  ``keep_device``: a third
    value, name -> tensor of the columns of ``<name>_analysed.csv`` that are on the device now -- the eight output columns
    and the four inputs they do not replace -- for ``helper_file.write_table_device``."""
    import torch
    n = len(df)
    L = _lib.lib()
    dev = torch.device(device)
    with _lib.on(dev):
        def up(name, dtype):
            return torch.from_numpy(np.ascontiguousarray(df[name].to_numpy(), dtype=dtype).view(
                np.int32 if dtype == np.uint32 else dtype)).to(dev)
        cols = columns_dev if columns_dev is not None else [
            up("TRACK_ID", np.uint32), up("POSITION_T", np.uint32), up("POSITION_X", np.float64),
            up("POSITION_Y", np.float64), up("WIDTH", np.float64), up("HEIGHT", np.float64)]
        if len(cols) != 6 or any(c.numel() != n or not c.is_cuda for c in cols):
            raise ValueError("columns_dev must be the table's six columns on {}".format(dev))
        ws = torch.empty(max(L.ysmr_evaluate_workspace_bytes(n), 256), dtype=torch.uint8, device=dev)
        f64 = lambda: torch.empty(max(n, 1), dtype=torch.float64, device=dev)   # noqa: E731
        i8 = lambda: torch.empty(max(n, 1), dtype=torch.int8, device=dev)       # noqa: E731
        out = {"WIDTH": f64(), "HEIGHT": f64(), "angle_diff": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
               "moving": i8(), "turn_points": i8(), "tp_of_tracks": f64(), "travelled_dist": f64(), "motility_phenotype": i8()}
        stats = torch.empty(max(n, 1), 12, dtype=torch.float64, device=dev)
        n_tracks = ctypes.c_longlong(0)
        rc = L.ysmr_evaluate_tracks(_lib.stream_ptr(dev), n, *[c.data_ptr() for c in cols], ctypes.byref(params), ws.data_ptr(),
                                    ws.numel(), out["WIDTH"].data_ptr(), out["HEIGHT"].data_ptr(), out["angle_diff"].data_ptr(),
                                    out["moving"].data_ptr(), out["turn_points"].data_ptr(), out["tp_of_tracks"].data_ptr(),
                                    out["travelled_dist"].data_ptr(), out["motility_phenotype"].data_ptr(), stats.data_ptr(),
                                    ctypes.byref(n_tracks))
        _lib.check(rc, "ysmr_evaluate_tracks")
        host = {k: v[:n].cpu().numpy() for k, v in out.items()}, stats[: n_tracks.value].cpu().numpy()
        if not keep_device:
            return host
        held = dict(zip(("TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y"), cols[:4]))
        held.update({k: v[:n] for k, v in out.items()})
        return host + (held,)


def evaluate_tracks(path_to_file, results_directory=None, df=None, settings=None, fps=None, device="cuda:0", **_):
    """Statistics of the selected tracks (track_eval.py:846-1318): returns ``(df, df_stats)`` -- the table with the
    per-row columns of ``<name>_analysed.csv`` and the per-track table of ``<name>_statistics.csv`` (plus its
    'Categories (...)' column, 'All', as upstream) -- or None after logging the reason."""
    import pandas as pd
    logger = logging.getLogger("ysmr").getChild(__name__)
    settings = get_configs(settings)
    if settings is None:
        logger.critical("No settings provided.")
        return None
    if fps is None or fps <= 0 or settings["force tracking.ini fps settings"]:
        fps = settings["frames per second"]
        if not fps > 0:
            logger.critical("fps value is negative or zero; cannot continue.")
            return None
    if results_directory is None:
        results_directory = create_results_folder(path_to_file)
    file_name = os.path.splitext(os.path.basename(path_to_file))[0]
    columns_dev = None
    if not isinstance(df, pd.DataFrame):
        if settings.get("hip read csv on device"):
            # text to numbers on the device (csrc/csv.hip); the columns stay there for the statistics
            table = read_table_device(path_to_file, device)
            df = None if table is None else table.to_dataframe()
            columns_dev = None if table is None else table.columns_dev
        else:
            df = get_data(path_to_file)
    if df is None:
        logger.critical("Error reading data frame from file {}".format(path_to_file))
        return None
    if len(df) == 0:
        logger.critical("Error reading data frame from file {}".format(path_to_file))
        return None
    table = df.reset_index(drop=True)
    first = table.groupby("TRACK_ID")["POSITION_T"].transform("first")
    if (table["POSITION_T"].astype(np.int64) < first.astype(np.int64)).any():
        logger.critical("POSITION_T contains negative values")
        return None
    try:
        # (the columns that came from the device a moment ago are not uploaded again)
        extra = {} if columns_dev is None else {"columns_dev": columns_dev}
        held = None
        if settings.get("hip write csv on device") and settings["store final analysed .csv file"]:
            # (... and what the analysed csv is printed from stays there)
            rows, stats, held = evaluate_columns(table, evaluate_params(settings, fps), device=device, keep_device=True, **extra)
        else:
            rows, stats = evaluate_columns(table, evaluate_params(settings, fps), device=device, **extra)
    except (_lib.YsmrLibraryError, RuntimeError) as exc:
        logger.critical("Device path failed for file {}: {}".format(path_to_file, exc))
        return None
    out = table.loc[:, ["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE"]].copy()
    for name in ("WIDTH", "HEIGHT", "angle_diff", "moving", "turn_points", "tp_of_tracks", "travelled_dist",
                 "motility_phenotype"):
        out[name] = rows[name]
    out = out.loc[:, ROW_COLUMNS]
    track_ids = stats[:, 10].astype(table["TRACK_ID"].dtype)
    index = pd.Index(track_ids, name="TRACK_ID")
    df_stats = pd.DataFrame({name: stats[:, k] for k, name in enumerate(STATS_COLUMNS)}, index=index)
    df_stats["Bacteria Length"] = df_stats["Bacteria Length"].astype(np.float32)     # (pandas' float16 group mean)
    df_stats["Motility Phenotype"] = df_stats["Motility Phenotype"].astype(np.int8)
    df_stats["TRACK_ID"] = track_ids
    save_path = os.path.join(results_directory, file_name) + "_{}{}"
    if settings["store generated statistical .csv file"]:
        save_df_to_csv(df=df_stats, save_path=save_path.format("statistics", ".csv"))
    share = [float((df_stats["Motility Phenotype"] == k).sum()) / len(df_stats) for k in (0, 1, 2)]
    logger.info("Nonmotile: {:.2%}, twitching: {:.2%}, motile: {:.2%}".format(*share))
    q1, q2, q3 = np.quantile(df_stats["Time (s)"], (0.25, 0.5, 0.75))
    logger.debug("Time duration of selected tracks min: {:.3f}, max: {:.3f}, Quantiles (25/50/75%): {:.3f}, {:.3f}, {:.3f}"
                 "".format(df_stats["Time (s)"].min(), df_stats["Time (s)"].max(), q1, q2, q3))
    # the category column the reference adds for its violin plots (track_eval.py:1150-1183)
    wanted = settings["split results by (Turn Points / Distance / Speed / Time / Displacement / perc. motile)"]
    parameter = next((name for name in STATS_COLUMNS if str(wanted).lower() in name.lower()), None)
    if not parameter:
        logger.warning("Setting 'split results by parameter (Turn Points / Distance / Speed / Time / Displacement / % motile)' "
                       "could not be assigned, reverted to 'perc. motile'.")
        parameter = STATS_COLUMNS[5]
    df_stats["Categories ({})".format(parameter)] = "All"
    violins = bool(settings.get("hip violin plots"))
    asked = [k for k in _SKIPPED_PLOT_KEYS if settings.get(k)]
    if asked and not violins:
        logger.info("Plots are not part of the HIP path; skipped: {}".format(", ".join(asked)))
    if settings["store final analysed .csv file"]:
        if held is not None:
            # numbers to text on the device (csrc/table_csv.hip): the same bytes; DEGREES_ANGLE is the one column uploaded
            write_table_device(out, save_path.format("analysed", ".csv"), device, columns_dev=held)
        else:
            save_df_to_csv(df=out, save_path=save_path.format("analysed", ".csv"))
    if violins or any(settings.get(k) for k in ("save large plots", "save rose plot", "save angle distribution plot / bins")):
        _figures(out, stats, settings, plot_title(file_name), save_path, device, logger, df_stats, parameter)
    logging.info("Done evaluating file {}".format(file_name))
    return out, df_stats
