"""Reading a track table back: helper_file.get_data through pandas.read_csv against helper_file.read_table_device (csrc/csv.hip),
end to end, in one warm process on one GPU.

Writes a list of about a million rows with the project's own formatter (the size of the bench clip's list), then ALTERNATES the
two paths, first for ``get_data`` alone, then for ``select_tracks(path_to_file=...)`` without and with 'hip read csv on device'.
Prints every round, the median and the spread of each path, and the device path's phases (file read, upload, index, parse,
order, download, DataFrame construction; ``sync_phases`` waits for the device between them, which the plain call does not).
The yardstick is the pandas path of the same process on the same file.

    python scripts/csv_read_e2e.py [--rows 1000000] [--rounds 7] [--shuffled]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_rows(n, rng, shuffled):
    from ysmr_amd import _lib
    per_track = 1000
    rows = np.zeros(n, _lib.ROW_DTYPE)
    ids = np.arange(n) // per_track
    rows["track_id"], rows["frame"] = ids, np.arange(n) % per_track
    start = rng.uniform((150, 120), (1100, 800), (ids[-1] + 1, 2))
    walk = rng.normal(0, 1.2, (n, 2))
    walk[::per_track] = 0.0
    pos = np.cumsum(walk, axis=0)
    pos -= np.repeat(pos[::per_track], per_track, axis=0)[:n]
    rows["x"], rows["y"] = (pos + start[ids]).T
    rows["w"], rows["h"] = rng.normal(6.0, 0.5, n).astype(np.float32), rng.normal(2.0, 0.2, n).astype(np.float32)
    rows["angle"] = rng.uniform(-90, 0, n).astype(np.float32)
    return rows[rng.permutation(n)] if shuffled else rows


def spread(name, values):
    print("{:<44s} median {:8.2f} ms   min {:8.2f}   max {:8.2f}   ({} rounds)".format(
        name, 1e3 * statistics.median(values), 1e3 * min(values), 1e3 * max(values), len(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shuffled", action="store_true", help="rows in random order: both paths sort")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import logging
    import torch
    from ysmr_amd import helper_file as hf
    from ysmr_amd.helper_file import default_settings, get_data, read_table_device, rows_to_csv_file
    from ysmr_amd.select import select_tracks
    logging.getLogger("ysmr").setLevel(logging.ERROR)
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, "bench_list.csv")
        n_bytes = rows_to_csv_file(make_rows(args.rows, rng, args.shuffled), path)
        print("{}: {} rows, {} bytes ({:.1f} per row), {}".format(os.path.basename(path), args.rows, n_bytes, n_bytes / args.rows,
                                                                 "shuffled" if args.shuffled else "in order"))
        print("device: {}".format(torch.cuda.get_device_name(torch.device(args.device))))

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        # ---- get_data alone ----
        _, ref = timed(lambda: get_data(path))
        _, got = timed(lambda: get_data(path, device=args.device))           # (warm: pinned buffers, code objects)
        table = read_table_device(path, args.device)
        assert table.path_taken == "device" and table.unserved == 0
        same = all(np.array_equal(got[c].to_numpy().view(np.uint32 if k < 2 else np.uint64), ref[c].to_numpy().view(np.uint32 if k < 2 else np.uint64))
                   for k, c in enumerate(ref.columns))
        print("the two DataFrames hold the same bits: {}".format(same and list(got.columns) == list(ref.columns) and got.index.equals(ref.index)))
        host, dev, phases = [], [], []
        for r in range(args.rounds):
            host.append(timed(lambda: get_data(path))[0])
            dev.append(timed(lambda: get_data(path, device=args.device))[0])
            t_ph, _ = timed(lambda: read_table_device(path, args.device, sync_phases=True).to_dataframe())
            marks = dict(hf.LAST_CSV_READ_MARKS)
            order = ["file read", "upload", "index", "parse", "order"]
            steps, before = {}, 0.0
            for k in order:
                if k in marks:
                    steps[k], before = marks[k] - before, marks[k]
            steps["download"], steps["DataFrame"], steps["all"] = marks["download"], marks["frame"] - marks["download"], t_ph
            phases.append(steps)
            print("round {}: get_data pandas {:8.2f} ms   device {:8.2f} ms   (with phase waits {:8.2f} ms)".format(
                r, 1e3 * host[-1], 1e3 * dev[-1], 1e3 * t_ph))
        spread("get_data, pandas.read_csv", host)
        spread("get_data, device", dev)
        for k in ["file read", "upload", "index", "parse", "order", "download", "DataFrame", "all"]:
            values = [p[k] for p in phases if k in p]
            if values:
                spread("  device phase: " + k, values)
        # ---- select_tracks(path_to_file=...) ----
        off = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                                  "minimal length in seconds": 20.0, "limit track length to x seconds": 20.0,
                                  "store processed .csv file": False, "frame height": 922, "frame width": 1228})
        on = dict(off, **{"hip read csv on device": True})
        kw = dict(path_to_file=path, results_directory=folder, fps=30.0, frame_height=922, frame_width=1228, device=args.device)
        a = select_tracks(settings=dict(off), **kw)
        b = select_tracks(settings=dict(on), **kw)
        print("select_tracks: {} rows selected; the same with the key: {}".format(
            None if a is None else len(a), (a is None and b is None) or (a is not None and b is not None and a.equals(b))))
        s_host, s_dev = [], []
        for r in range(args.rounds):
            s_host.append(timed(lambda: select_tracks(settings=dict(off), **kw))[0])
            s_dev.append(timed(lambda: select_tracks(settings=dict(on), **kw))[0])
            print("round {}: select_tracks pandas {:8.2f} ms   device {:8.2f} ms".format(r, 1e3 * s_host[-1], 1e3 * s_dev[-1]))
        spread("select_tracks, pandas.read_csv", s_host)
        spread("select_tracks, 'hip read csv on device'", s_dev)


if __name__ == "__main__":
    main()
