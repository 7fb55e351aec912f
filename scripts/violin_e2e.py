"""The violin plots end to end: evaluate_tracks on the selected table of a synthetic clip with 'hip violin plots' on and
off (the eight figures must be there), then one figure's phases -- statistics and densities on the device, profile and
paint with the canvas download, lettering, PNG -- for per-track tables of 500 and 20 000 tracks.  Not compared with
upstream: seaborn is needed for that.

  python3 scripts/violin_e2e.py [--frames 600] [--tmp DIR] [--png host|device] > profiles/violin_e2e.log
  python3 scripts/violin_e2e.py --png-ab >> profiles/png_dynamic_e2e.log     (only the three PNG paths -- host, device, device 'dynamic' --
                                                                              alternating: times and sizes)
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FIGURES = ("turning_points", "distance", "speed", "time_plot", "displacement", "perc_motile", "arc-chord_ratio", "Median_speed")


def statistics_table(n_tracks, seed=0):
    """A per-track table as evaluate_tracks builds it, filled with plausible numbers."""
    import pandas as pd
    from ysmr_amd.evaluate import STATS_COLUMNS
    rng = np.random.default_rng(seed)
    cols = {name: rng.gamma(2.0, 3.0, n_tracks) for name in STATS_COLUMNS}
    cols["Perc. Motile"] = np.round(rng.uniform(0.0, 100.0, n_tracks), 2)
    cols["Arc-Chord Ratio"] = rng.uniform(0.0, 1.0, n_tracks)
    cols["Motility Phenotype"] = rng.integers(0, 3, n_tracks).astype(np.float64)
    cols["TRACK_ID"] = np.arange(n_tracks, dtype=np.float64)
    return pd.DataFrame(cols)


def figure_phases(n_tracks, work, reps, on_device=False):
    import torch
    from plots_e2e import timed
    from ysmr_amd import _lib, plot_functions as pf
    from ysmr_amd.evaluate import violin_cut_list
    dev = torch.device("cuda:0")
    table = statistics_table(n_tracks)
    cut_list = violin_cut_list("Perc. Motile", [0.0, 20.0, 40.0, 60.0, 80.0, 100.01])
    labels = [name for _, _, name in cut_list]
    lo, hi = [a for a, _, _ in cut_list[1:]], [b for _, b, _ in cut_list[1:]]
    cut, value = table["Perc. Motile"].to_numpy(), table["Speed (µm/s)"].to_numpy()
    path = os.path.join(work, "violin_{}.png".format(n_tracks))
    for rep in range(reps):
        with _lib.on(dev):
            (sums, dens), t_stats = timed(lambda: pf.device_violin_stats(cut, value, lo, hi, dev))
            view, rows = pf.violin_view(sums, 0.0, False)
            rgb_dev, t_paint = timed(lambda: pf.device_violins(sums, dens, view, dev, download=False))
            rgb, t_down = timed(lambda: rgb_dev.cpu().numpy())
        t0 = time.perf_counter()
        pf.decorate_violin_figure(rgb, view, rows, "bench clip", "Speed (µm/s)", labels, pf.violin_text_boxes(sums, labels))
        t_text = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        pf.write_png(path, rgb)
        t_png = (time.perf_counter() - t0) * 1e3
        _, t_all = timed(lambda: pf.violin_plot(table, path, "Speed (µm/s)", "Categories (Perc. Motile)", cut_list, "bench clip", 0.0, False,
                                                png_on_device=on_device))
        print("rep {}: {:6d} tracks: statistics and densities (upload, sort, kernels, download) {:6.2f} ms, profile and paint {:5.2f} ms, "
              "download {:5.2f} ms, lettering {:5.2f} ms, png {:5.1f} ms; violin_plot (png on the {}) {:6.1f} ms ({:.2f} MB)".format(
                  rep, n_tracks, t_stats, t_paint, t_down, t_text, t_png, "device" if on_device else "host", t_all,
                  os.path.getsize(path) / 1e6), flush=True)


def violin_figures(n_tracks):
    from ysmr_amd import plot_functions as pf
    from ysmr_amd.evaluate import violin_cut_list
    table = statistics_table(n_tracks)
    cut_list = violin_cut_list("Perc. Motile", [0.0, 20.0, 40.0, 60.0, 80.0, 100.01])
    return [("violin_{}".format(n_tracks), lambda path, dev: pf.violin_plot(table, path, "Speed (µm/s)", "Categories (Perc. Motile)", cut_list,
                                                                            "bench clip", 0.0, False, png_on_device=dev))]


def run(args):
    from plots_e2e import selected_table, timed
    from ysmr_amd.evaluate import evaluate_tracks
    from ysmr_amd.helper_file import default_settings
    work = tempfile.mkdtemp(prefix="violin_e2e_", dir=args.tmp)
    try:
        base = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                                   "save large plots": False, "save rose plot": False, "save angle distribution plot / bins": 0})
        on = dict(base, **{"hip violin plots": True})
        if args.png_ab:
            from plots_e2e import png_ab
            for n_tracks in (500, 20000):
                png_ab(violin_figures(n_tracks), work, args.reps)
            return 0
        if args.png == "device":
            on["hip png on device"] = True
        table, fps = selected_table(args, work, base)
        name = os.path.join(work, "clip_selected_data.csv")
        evaluate_tracks(name, work, df=table, settings=base, fps=fps)                   # warm-up: library, allocator
        for rep in range(args.reps):
            _, t_on = timed(lambda: evaluate_tracks(name, work, df=table, settings=on, fps=fps))
            _, t_off = timed(lambda: evaluate_tracks(name, work, df=table, settings=base, fps=fps))
            print("rep {}: evaluate_tracks with the eight violin figures {:.1f} ms, without {:.1f} ms".format(rep, t_on, t_off), flush=True)
        missing = [f for f in FIGURES if not os.path.exists(os.path.join(work, "clip_selected_data_{}.png".format(f)))]
        print("figures written: {} of {}{}".format(len(FIGURES) - len(missing), len(FIGURES), ", missing: {}".format(missing) if missing else ""))
        for n_tracks in (500, 20000):
            figure_phases(n_tracks, work, args.reps, on_device=args.png == "device")
        print("not compared with upstream: seaborn is not installed here")
        return 1 if missing else 0
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--height", type=int, default=922)
    ap.add_argument("--width", type=int, default=1228)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="where the clip and the figures go (removed afterwards)")
    ap.add_argument("--png", choices=("host", "device"), default="host", help="where the PNG files are made ('hip png on device')")
    ap.add_argument("--png-ab", action="store_true", help="only compare the three PNG paths: times, file sizes, zlib level 1")
    sys.exit(run(ap.parse_args()))
