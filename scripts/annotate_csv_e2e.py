"""annotate_video handed the path of an ``*_analysed.csv``: the table through pandas.read_csv and annotate.build_marks against
'hip read csv on device' (csrc/csv.hip: ysmr_csv_parse_typed; csrc/marks.hip: ysmr_marks_build), end to end, in one warm
process on one GPU.

Writes an analysed csv of about a million rows (the thirteen columns of evaluate_tracks, its dtypes, empty cells where a
position or a turning-point rate is missing) with the project's own writer, and a short gray clip; then ALTERNATES the two table
paths.  Per round and path it prints the time from the call to "marks on the device" (annotate.LAST_MARKS_TIMES: on the host
path behind the upload of the finished arrays, on the device path behind the download of the mark count) and the whole call;
then best, median and range of each.  The two files are compared byte for byte.  The yardstick is the host path of the same
process on the same file.

    python scripts/annotate_csv_e2e.py [--rows 1000000] [--frames 1920] [--rounds 5] [--shuffled] [--mjpeg]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_table(n, n_frames, height, width, rng, shuffled):
    """Tracks of n_frames / 2 rows each, in evaluate_tracks' order (by track, then frame)."""
    import pandas as pd
    per_track = max(1, n_frames // 2)
    ids = np.arange(n) // per_track
    start_frame = rng.integers(0, n_frames - per_track + 1, ids[-1] + 1)
    start = rng.uniform((0, 0), (width, height), (ids[-1] + 1, 2))
    walk = rng.normal(0, 1.2, (n, 2))
    walk[::per_track] = 0.0
    pos = np.cumsum(walk, axis=0)
    pos -= np.repeat(pos[::per_track], per_track, axis=0)[:n]
    x, y = (pos + start[ids]).T.copy()
    x[rng.random(n) < 0.01] = np.nan
    tp = rng.uniform(0, 3, n)
    tp[rng.random(n) < 0.5] = np.nan
    df = pd.DataFrame({
        "TRACK_ID": ids.astype(np.uint32), "POSITION_T": (start_frame[ids] + np.arange(n) % per_track).astype(np.uint32),
        "POSITION_X": x, "POSITION_Y": y, "WIDTH": rng.normal(6.0, 0.5, n), "HEIGHT": rng.normal(2.0, 0.2, n),
        "DEGREES_ANGLE": rng.uniform(-90, 0, n), "angle_diff": rng.uniform(-90, 90, n),
        "moving": (rng.random(n) < 0.7).astype(np.int8), "turn_points": (rng.random(n) < 0.1).astype(np.int8),
        "tp_of_tracks": tp, "travelled_dist": rng.uniform(0, 40, n), "motility_phenotype": rng.integers(0, 3, ids[-1] + 1).astype(np.int8)[ids]})
    return df.iloc[rng.permutation(n)].reset_index(drop=True) if shuffled else df


def spread(name, values):
    print("{:<56s} best {:8.2f} ms   median {:8.2f}   max {:8.2f}   ({} rounds)".format(
        name, 1e3 * min(values), 1e3 * statistics.median(values), 1e3 * max(values), len(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=1920)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shuffled", action="store_true", help="rows in random order: both paths sort the table")
    ap.add_argument("--mjpeg", action="store_true", help="write Motion-JPEG instead of the uncompressed AVI")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import logging
    import torch
    from ysmr_amd import annotate
    from ysmr_amd.helper_file import default_settings, write_table_device
    logging.getLogger("ysmr").setLevel(logging.ERROR)
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as folder:
        clip = os.path.join(folder, "clip.npy")
        np.save(clip, rng.integers(0, 200, (args.frames, args.height, args.width), dtype=np.uint8))
        csv = os.path.join(folder, "clip_analysed.csv")
        wrote = write_table_device(make_table(args.rows, args.frames, args.height, args.width, rng, args.shuffled), csv, args.device, rename_old_file=False)
        print("{}: {} rows, {} bytes, written on the {}, {}".format(os.path.basename(csv), args.rows, os.path.getsize(csv), wrote,
                                                                  "shuffled" if args.shuffled else "in track order"))
        print("clip: {} frames of {} x {}, gray; output: {}".format(args.frames, args.width, args.height,
                                                                   "Motion-JPEG" if args.mjpeg else "uncompressed 24-bit AVI"))
        print("device: {}".format(torch.cuda.get_device_name(torch.device(args.device))))
        off = default_settings(**{"log to file": False, "log_level": logging.ERROR, "frames per second": 30.0, "save video file extension": ".avi",
                                  "save video fourcc codec": "MJPG" if args.mjpeg else "DIB "})
        on = dict(off, **{"hip read csv on device": True})

        def call(settings, name):
            out = os.path.join(folder, name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            written = annotate.annotate_video(clip, csv, settings=dict(settings), result_folder=out, device=args.device)
            torch.cuda.synchronize()
            whole = time.perf_counter() - t0
            assert written is not None, "annotate_video failed"
            return whole, annotate.LAST_MARKS_TIMES["marks on device"], dict(annotate.LAST_MARKS), written

        _w, _t, went_host, file_host = call(off, "host")                  # (warm: pinned buffers, code objects, the page cache)
        _w, _t, went_dev, file_dev = call(on, "device")
        assert went_host["path"] == "host" and went_dev["path"] == "device", (went_host, went_dev)
        with open(file_host, "rb") as a, open(file_dev, "rb") as b:
            same = a.read() == b.read()
        print("marks: {} of {} rows on both paths: {}; the two files hold the same bytes: {}".format(
            went_dev["marks"], went_dev["rows"], went_dev == dict(went_host, path="device"), same))
        whole = {"host": [], "device": []}
        table = {"host": [], "device": []}
        for r in range(args.rounds):
            for name, settings in (("host", off), ("device", on)):
                w, t, went, _f = call(settings, name)
                assert went["path"] == name
                whole[name].append(w)
                table[name].append(t)
            print("round {}: marks on the device after  pandas + build_marks {:8.2f} ms   device {:8.2f} ms;   whole call {:8.2f} ms   {:8.2f} ms".format(
                r, 1e3 * table["host"][-1], 1e3 * table["device"][-1], 1e3 * whole["host"][-1], 1e3 * whole["device"][-1]))
        spread("call -> marks on the device, pandas + build_marks", table["host"])
        spread("call -> marks on the device, 'hip read csv on device'", table["device"])
        spread("whole annotate_video, pandas + build_marks", whole["host"])
        spread("whole annotate_video, 'hip read csv on device'", whole["device"])
        spread("  of it the video pass, host table path", [w - t for w, t in zip(whole["host"], table["host"])])
        spread("  of it the video pass, device table path", [w - t for w, t in zip(whole["device"], table["device"])])


if __name__ == "__main__":
    main()
