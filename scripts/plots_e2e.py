"""The three track figures end to end on the selected table of the bench clip (1228 x 922, 500 blobs, 1920 frames):
per figure the device time (upload of the small arrays, kernels), the canvas download, the lettering + PNG encoding and
the wall time of the public function; the matplotlib scatter loop of the reference's overview on the same table where
matplotlib is importable; evaluate_tracks with the three keys on and off.  ``--png device`` runs the public functions and
evaluate_tracks with 'hip png on device'; ``--png-ab`` runs only the comparison of the three PNG paths (host, device with
the fixed code, device with 'dynamic'): per figure the wall time of the public function on every path, alternating, the
file sizes, and zlib level 1 on the same scanlines.

  python3 scripts/plots_e2e.py [--frames 1920] [--tmp DIR] [--png host|device] > profiles/plots_e2e.log
  python3 scripts/plots_e2e.py --frames 600 --png-ab >> profiles/png_dynamic_e2e.log
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def selected_table(args, work, settings):
    import torch
    from ysmr_amd.select import select_tracks
    from ysmr_amd.synth import SyntheticVideo
    from ysmr_amd.track_eval import track_bacteria
    t0 = time.perf_counter()
    path = os.path.join(work, "clip.npy")
    np.save(path, SyntheticVideo(args.height, args.width, args.blobs, seed=0).frames(args.frames))
    print("clip: {} frames of {} x {}, {} blobs, generated in {:.1f} s".format(args.frames, args.width, args.height, args.blobs,
                                                                             time.perf_counter() - t0), flush=True)
    df, fps, height, width, _ = track_bacteria(path, settings=dict(settings), result_folder=work)
    torch.cuda.synchronize()
    selected = select_tracks(path_to_file=path, df=df, results_directory=work, fps=fps, frame_height=height, frame_width=width,
                             settings=dict(settings))
    if selected is None or len(selected) == 0:
        print("select_tracks kept nothing of this clip: the figures are drawn from the whole tracked table", flush=True)
        selected = df
    print("table: {} rows in {} tracks (tracked: {} rows)".format(len(selected), selected["TRACK_ID"].nunique(), len(df)), flush=True)
    return selected.reset_index(drop=True), fps


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def figure_phases(out, stats, settings, work, reps):
    """Device / download / encode per figure, the steps of plot_functions' public functions taken one at a time."""
    import torch
    from ysmr_amd import _lib, plot_functions as pf
    dev = torch.device("cuda:0")
    px, lag, bins = settings["pixel per micrometre"], settings["compare angle between n frames"], 36
    dist = np.ascontiguousarray(stats["Distance (µm)"].to_numpy())
    W, H = pf.canvas_size(300)
    for rep in range(reps):
        with _lib.on(dev):
            (ids, x, y, moving), t_up = timed(lambda: pf._upload(out, dev, moving=True))
            print("rep {}: upload of the four columns {:.2f} ms".format(rep, t_up))
            for mode, name in ((0, "Bac_Run_Overview"), (1, "rose_graph")):
                ext, t_ext = timed(lambda: pf.device_extent(ids, x, y, mode, px, dev))
                view, cols, rows = pf.track_view(ext, mode, px)
                rgb_dev, t_paint = timed(lambda: pf.device_tracks(ids, x, y, dist, view, dev, download=False))
                rgb, t_down = timed(lambda: rgb_dev.cpu().numpy())
                t0 = time.perf_counter()
                pf.decorate_track_figure(rgb, view, cols, rows, "bench clip", float(dist.min()), float(dist.max()))
                t_text = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                pf.write_png(os.path.join(work, name + "_phases.png"), rgb)
                t_png = (time.perf_counter() - t0) * 1e3
                print("rep {}: {:17s} extent {:6.2f} ms, paint (workspace + kernels) {:6.2f} ms, download {:6.2f} ms, lettering {:5.2f} ms, "
                      "png {:6.1f} ms ({:.2f} MB)".format(rep, name, t_ext, t_paint, t_down, t_text, t_png,
                                                          os.path.getsize(os.path.join(work, name + "_phases.png")) / 1e6))
            edges = np.linspace(-np.pi, np.pi, bins + 1)
            (counts, points), t_hist = timed(lambda: pf.device_angle_histogram(ids, x, y, moving, lag, edges, dev))
            dirs, bin_of = pf.wedge_boundaries(edges)
            cx, cy, ring_r2, r2 = pf.wedge_plan(counts[bin_of], W, H)
            rgb_dev, t_paint = timed(lambda: pf.device_wedges(W, H, cx, cy, dirs, r2, ring_r2, dev, download=False))
            rgb, t_down = timed(lambda: rgb_dev.cpu().numpy())
            t0 = time.perf_counter()
            pf.write_png(os.path.join(work, "angle_phases.png"), rgb)
            t_png = (time.perf_counter() - t0) * 1e3
            print("rep {}: {:17s} histogram {:6.2f} ms ({} points), wedges {:6.2f} ms, download {:6.2f} ms, png {:6.1f} ms".format(
                rep, "angle_histogram", t_hist, points, t_paint, t_down, t_png))


def public_functions(out, stats, settings, work, reps, on_device=False):
    from ysmr_amd import plot_functions as pf
    dist = np.ascontiguousarray(stats["Distance (µm)"].to_numpy())
    px = settings["pixel per micrometre"]
    for rep in range(reps):
        _, a = timed(lambda: pf.large_xy_plot(out, "bench clip", os.path.join(work, "overview.png"), px_to_micrometre=px, distances=dist,
                                              dist_min=float(dist.min()), dist_max=float(dist.max()), png_on_device=on_device))
        _, b = timed(lambda: pf.rose_graph(out, "bench clip", os.path.join(work, "rose.png"), px_to_micrometre=px, distances=dist,
                                           dist_min=float(dist.min()), dist_max=float(dist.max()), png_on_device=on_device))
        _, c = timed(lambda: pf.angle_distribution_plot(out, 36, "bench clip", os.path.join(work, "angle.png"),
                                                        compare_n_frames=settings["compare angle between n frames"], png_on_device=on_device))
        print("rep {} (png on the {}): wall time large_xy_plot {:.1f} ms, rose_graph {:.1f} ms, angle_distribution_plot {:.1f} ms".format(
            rep, "device" if on_device else "host", a, b, c))


def read_scanlines(path):
    """(IHDR body, the inflated IDAT) of a PNG written by write_png / write_png_device."""
    import struct
    import zlib
    raw = open(path, "rb").read()
    at, head, idat = 8, None, b""
    while at < len(raw):
        (size,) = struct.unpack(">I", raw[at:at + 4])
        kind, body = raw[at + 4:at + 8], raw[at + 8:at + 8 + size]
        head = body if kind == b"IHDR" else head
        idat += body if kind == b"IDAT" else b""
        at += 12 + size
    return head, zlib.decompress(idat)


def png_ab(figures, work, reps):
    """``figures``: (name, draw(path, png_on_device)).  Per figure and repetition the wall time of ``draw`` on the host path,
    on the device path with the fixed code and on the device path with the dynamic code ('dynamic'), one after the other;
    then the three files' sizes, zlib level 1 on the same scanlines (what the host path's IDAT is) and whether the three
    files hold the same pixels."""
    import zlib
    for name, draw in figures:
        host, device, dynamic = (os.path.join(work, name + tail) for tail in ("_host.png", "_device.png", "_dynamic.png"))
        draw(host, False), draw(device, True), draw(dynamic, "dynamic")                # warm-up of every path
        for rep in range(reps):
            _, t_host = timed(lambda: draw(host, False))
            _, t_dev = timed(lambda: draw(device, True))
            _, t_dyn = timed(lambda: draw(dynamic, "dynamic"))
            print("rep {}: {:17s} wall time, png on the host {:7.1f} ms, on the device {:7.1f} ms, on the device 'dynamic' {:7.1f} ms".format(
                rep, name, t_host, t_dev, t_dyn), flush=True)
        (head_h, raw_h), (head_d, raw_d), (head_y, raw_y) = read_scanlines(host), read_scanlines(device), read_scanlines(dynamic)
        t0 = time.perf_counter()
        level1 = len(zlib.compress(raw_h, 1))
        t_zlib = (time.perf_counter() - t0) * 1e3
        sizes = [os.path.getsize(f) for f in (host, device, dynamic)]
        print("       {:17s} files: host {} bytes, device {} bytes (ratio {:.3f}), device 'dynamic' {} bytes (ratio {:.3f}); zlib level 1 on the "
              "{:.1f} MB of scanlines: {} bytes in {:.1f} ms on this host's CPU; same header and pixels: {}".format(
                  name, sizes[0], sizes[1], sizes[1] / sizes[0], sizes[2], sizes[2] / sizes[0], len(raw_h) / 1e6, level1, t_zlib,
                  head_h == head_d == head_y and raw_h == raw_d == raw_y), flush=True)


def track_figures(out, stats, settings):
    from ysmr_amd import plot_functions as pf
    dist = np.ascontiguousarray(stats["Distance (µm)"].to_numpy())
    px, span = settings["pixel per micrometre"], dict(dist_min=float(dist.min()), dist_max=float(dist.max()))
    return [("Bac_Run_Overview", lambda path, dev: pf.large_xy_plot(out, "bench clip", path, px_to_micrometre=px, distances=dist,
                                                                    png_on_device=dev, **span)),
            ("rose_graph", lambda path, dev: pf.rose_graph(out, "bench clip", path, px_to_micrometre=px, distances=dist, png_on_device=dev,
                                                           **span)),
            ("angle_histogram", lambda path, dev: pf.angle_distribution_plot(
                out, 36, "bench clip", path, compare_n_frames=settings["compare angle between n frames"], png_on_device=dev))]


def device_png_phases(out, stats, settings, reps):
    """The device path's own steps on the overview's canvas: lettering (upload + kernel), deflate (kernels + the two downloads)."""
    import torch
    from ysmr_amd import _lib, plot_functions as pf
    dev = torch.device("cuda:0")
    px = settings["pixel per micrometre"]
    dist = np.ascontiguousarray(stats["Distance (µm)"].to_numpy())
    with _lib.on(dev):
        ids, x, y = pf._upload(out, dev)
        view, cols, rows = pf.track_view(pf.device_extent(ids, x, y, 0, px, dev), 0, px)
        rgb = pf.device_tracks(ids, x, y, dist, view, dev, download=False)
        stamps = pf.StampList(rgb.shape[0], rgb.shape[1])
        pf.decorate_track_figure(stamps, view, cols, rows, "bench clip", float(dist.min()), float(dist.max()))
        for rep in range(reps + 1):
            _, t_stamp = timed(lambda: pf.device_stamp(rgb, stamps))
            stream, t_deflate = timed(lambda: pf.device_deflate(rgb))
            dynamic, t_dynamic = timed(lambda: pf.device_deflate(rgb, dynamic=True))
            if rep:
                print("rep {}: overview canvas: ysmr_plot_stamp of {} records {:.2f} ms, ysmr_png_deflate with its downloads {:.2f} ms "
                      "({} bytes), ysmr_png_deflate_dynamic with its downloads {:.2f} ms ({} bytes)".format(
                          rep - 1, len(stamps.records), t_stamp, t_deflate, len(stream), t_dynamic, len(dynamic)), flush=True)


def matplotlib_loop(out, stats, settings, work):
    """The reference's overview as it draws it: one scatter call per track at 300 dpi (plot_functions.py:109-188)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib is not importable on this host: the host-side figure of comparison stays the 5.1 s measured on the "
              "development container (CPU, matplotlib 3.10.8, Agg, 500 tracks x 600 rows)")
        return
    px = settings["pixel per micrometre"]
    dist = stats["Distance (µm)"].to_numpy()
    c = (dist - dist.min()) / max(dist.max() - dist.min(), 1e-300)
    t0 = time.perf_counter()
    f = plt.figure()
    f.set_size_inches(11.6929133858, 8.2677165354)
    ax = f.add_subplot(1, 1, 1)
    for k, (_, g) in enumerate(out.groupby("TRACK_ID", sort=False)):
        ax.scatter(g["POSITION_X"] / px, g["POSITION_Y"] / px, marker=".", c=[plt.cm.viridis_r(c[k])] * len(g), s=1, lw=0)
    ax.set_aspect("equal")
    ax.grid(True)
    plt.savefig(os.path.join(work, "mpl.png"), dpi=300)
    plt.close()
    print("matplotlib {} on this host: one scatter call per track, {} tracks, {} rows: {:.2f} s".format(
        matplotlib.__version__, len(dist), len(out), time.perf_counter() - t0))


def run(args):
    from ysmr_amd.evaluate import evaluate_tracks
    from ysmr_amd.helper_file import default_settings
    work = tempfile.mkdtemp(prefix="plots_e2e_", dir=args.tmp)
    try:
        base = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False})
        off = dict(base, **{"save large plots": False, "save rose plot": False, "save angle distribution plot / bins": 0})
        table, fps = selected_table(args, work, base)
        name = os.path.join(work, "clip_selected_data.csv")
        evaluate_tracks(name, work, df=table, settings=off, fps=fps)                    # warm-up: library, allocator
        if args.png_ab:
            on_dev = dict(base, **{"hip png on device": True})
            res_on = evaluate_tracks(name, work, df=table, settings=on_dev, fps=fps)
            for rep in range(args.reps):
                _, t_host = timed(lambda: evaluate_tracks(name, work, df=table, settings=base, fps=fps))
                _, t_dev = timed(lambda: evaluate_tracks(name, work, df=table, settings=on_dev, fps=fps))
                _, t_off = timed(lambda: evaluate_tracks(name, work, df=table, settings=off, fps=fps))
                print("rep {}: evaluate_tracks with the three figures, png on the host {:.1f} ms, on the device {:.1f} ms, without figures "
                      "{:.1f} ms".format(rep, t_host, t_dev, t_off), flush=True)
            png_ab(track_figures(*res_on, base), work, args.reps)
            device_png_phases(*res_on, base, args.reps)
            return
        if args.png == "device":
            base = dict(base, **{"hip png on device": True})
        for rep in range(args.reps):
            (res_on), t_on = timed(lambda: evaluate_tracks(name, work, df=table, settings=base, fps=fps))
            (res_off), t_off = timed(lambda: evaluate_tracks(name, work, df=table, settings=off, fps=fps))
            print("rep {}: evaluate_tracks with the three figures {:.1f} ms, without {:.1f} ms".format(rep, t_on, t_off), flush=True)
        out, stats = res_on
        figure_phases(out, stats, base, work, args.reps)
        public_functions(out, stats, base, work, args.reps, on_device=args.png == "device")
        matplotlib_loop(out, stats, base, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1920)
    ap.add_argument("--height", type=int, default=922)
    ap.add_argument("--width", type=int, default=1228)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="where the clip and the figures go (removed afterwards)")
    ap.add_argument("--png", choices=("host", "device"), default="host", help="where the PNG files are made ('hip png on device')")
    ap.add_argument("--png-ab", action="store_true", help="only compare the three PNG paths: times, file sizes, zlib level 1")
    run(ap.parse_args())
