"""The collated workbook end to end: helper_file.collate_results_csv_to_xlsx with its sheets built on the device (csrc/csv.hip,
csrc/xlsx.hip) against its own host path (pandas.read_csv and a Python loop over the cells), in one warm process on one GPU.

Two cases: a result folder of 200 ``<name>_statistics.csv`` of 300 tracks each, in the shape ``evaluate_tracks`` writes (its
header holds the µ of 'Distance (µm)'), and ONE ``*_analysed.csv`` of a million rows by thirteen columns
(``csv_extension='analysed.csv'``).  The two paths ALTERNATE; every round is printed, then median and range per path and the
device path's phases summed over the files (file read, upload, index + kinds, parse, print, download, zip), and whether the
two workbooks are the same bytes.  The host path is the only yardstick there is: upstream's writer (xlsxwriter) is no dependency
of this project, so no figure for it is taken here.

    python scripts/xlsx_e2e.py [--files 200] [--tracks 300] [--rows 1000000] [--rounds 5] [--host-rounds-large 1]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ["file read", "upload", "index + kinds", "parse", "print", "download", "zip", "host sheet"]


def statistics_table(n, rng):
    from ysmr_amd.evaluate import STATS_COLUMNS
    df = pd.DataFrame({name: rng.uniform(0.0, 90.0, n) for name in STATS_COLUMNS})
    for name in STATS_COLUMNS:
        if "Phenotype" in name:
            df[name] = rng.integers(0, 3, n).astype(np.int8)
        elif "Length" in name:
            df[name] = rng.uniform(2, 9, n).astype(np.float32)
    df["TRACK_ID"] = np.arange(n, dtype=np.int64) * 3 + 1
    return df


def analysed_table(n, rng):
    tp = rng.uniform(0, 3, n)
    tp[rng.random(n) < 0.5] = np.nan
    dist = rng.uniform(0, 50, n)
    tiny = rng.random(n) < 0.02
    dist[tiny] = rng.normal(0, 1e-14, int(tiny.sum()))                  # (stationary tracks' rounding noise: cells of the wide printer)
    return pd.DataFrame({
        "TRACK_ID": np.arange(n, dtype=np.int64) // 1000, "POSITION_T": np.arange(n, dtype=np.int64) % 1000,
        "POSITION_X": rng.uniform(0, 1228, n), "POSITION_Y": rng.uniform(0, 922, n), "WIDTH": rng.uniform(2, 9, n),
        "HEIGHT": rng.uniform(9, 30, n), "DEGREES_ANGLE": rng.uniform(0, 180, n), "angle_diff": rng.integers(-90, 91, n),
        "moving": (rng.random(n) < 0.7).astype(np.int8), "turn_points": (rng.random(n) < 0.2).astype(np.int8),
        "tp_of_tracks": tp, "travelled_dist": dist, "motility_phenotype": rng.integers(0, 3, n).astype(np.int8)})


def spread(name, values):
    print("{:<44s} median {:9.2f} ms   min {:9.2f}   max {:9.2f}   ({} rounds)".format(
        name, 1e3 * statistics.median(values), 1e3 * min(values), 1e3 * max(values), len(values)))


def case(title, folder, extension, rounds, host_rounds, device, compress):
    import torch
    from ysmr_amd import helper_file as hf
    out = os.path.join(folder, "out")
    os.makedirs(out, exist_ok=True)

    def run(dev):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        book = hf.collate_results_csv_to_xlsx(folder, out, csv_extension=extension, device=dev, compress=compress)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        with open(book, "rb") as fh:
            data = fh.read()
        os.remove(book)
        return seconds, data, dict(hf.LAST_COLLATE), dict(hf.LAST_COLLATE_TIMES)
    files = hf.find_paths(folder, extension)
    print("\n== {}: {} file(s), {:.1f} MB of csv, {} entries ==".format(
        title, len(files), sum(os.path.getsize(p) for p in files) / 1e6, "deflated" if compress else "stored"))
    _, book_dev, taken, _ = run(device)                                      # (warm: pinned buffers, code objects)
    print("sheets built on the device: {} of {}".format(sum(v == "device" for v in taken.values()), len(taken)))
    host, dev, phases, book_host = [], [], [], None
    for r in range(rounds):
        line = "round {}:".format(r)
        if r < host_rounds:
            seconds, book_host, _, times = run(None)
            host.append(seconds)
            line += "  host {:9.2f} ms (sheets {:9.2f}, zip {:8.2f})".format(1e3 * seconds, 1e3 * times.get("host sheet", 0.0), 1e3 * times.get("zip", 0.0))
        seconds, data, _, times = run(device)
        dev.append(seconds)
        phases.append(times)
        assert data == book_dev, "two device runs gave different workbooks"
        print(line + "  device {:9.2f} ms".format(1e3 * seconds))
    print("workbook: {:.1f} MB; device and host path wrote the same bytes: {}".format(len(book_dev) / 1e6, book_host == book_dev))
    spread("collate, host path", host)
    spread("collate, device path", dev)
    for k in PHASES:
        values = [p[k] for p in phases if k in p]
        if values:
            spread("  device path, phase: " + k, values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--tracks", type=int, default=300)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds-large", type=int, default=1, help="host rounds of the million-row case (a Python cell loop: minutes)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--deflate", action="store_true")
    args = ap.parse_args()
    import logging
    import torch
    logging.getLogger("ysmr").setLevel(logging.ERROR)
    rng = np.random.default_rng(1)
    print("device: {}; pandas {}".format(torch.cuda.get_device_name(torch.device(args.device)), pd.__version__))
    with tempfile.TemporaryDirectory() as folder:
        for k in range(args.files):
            statistics_table(args.tracks, rng).to_csv(os.path.join(folder, "video_{:03d}_statistics.csv".format(k)), index=False)
        case("a result folder of statistics files", folder, "statistics.csv", args.rounds, args.rounds, args.device, args.deflate)
    with tempfile.TemporaryDirectory() as folder:
        analysed_table(args.rows, rng).to_csv(os.path.join(folder, "clip_analysed.csv"), index=False)
        case("one analysed csv", folder, "analysed.csv", args.rounds, args.host_rounds_large, args.device, args.deflate)


if __name__ == "__main__":
    main()
