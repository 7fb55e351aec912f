"""Writing the selection's and the analysis' tables: helper_file.save_df_to_csv (DataFrame.to_csv) against
helper_file.write_table_device (csrc/table_csv.hip), end to end, in one warm process on one GPU.

Builds a list of about a million rows with a share of stationary tracks (positions that move by rounding noise only, so that
``travelled_dist`` holds 1e-14-sized values and ``tp_of_tracks`` NaN -- the cells the fast float printer declines), takes the
table of ``<name>_selected_data.csv``'s shape from it and the table of ``<name>_analysed.csv`` from ``evaluate_tracks``, then
ALTERNATES the two writers on the same tables, and ``select_tracks`` / ``evaluate_tracks`` without and with
'hip write csv on device'.  Prints every round, the median and the range of each path, the device writer's steps (upload, the
device call -- pre-pass, wide cells, row printer, scans and packing launch in one call --, download, file write) and, as the
yardstick of the format step, the device time of ``ysmr_rows_format_device`` on the same number of rows next to the device time
of ``ysmr_table_format_device``, both between two events.  The files go to a temporary folder: the page cache takes them.

    python scripts/csv_write_e2e.py [--rows 1000000] [--rounds 5] [--still 0.25]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_list(n, rng, still):
    """A list's DataFrame: tracks of 1000 rows, random walks; a share `still` of them stands still but for steps of a few
    2^-44 px."""
    import pandas as pd
    per_track = 1000
    ids = np.arange(n) // per_track
    n_tracks = int(ids[-1]) + 1
    start = rng.uniform((150, 120), (1100, 800), (n_tracks, 2))
    walk = rng.normal(0, 1.2, (n, 2))
    quiet = rng.random(n_tracks) < still
    noise = rng.integers(-2, 3, (n, 2)) * 2.0 ** -44
    walk = np.where(quiet[ids][:, None], noise, walk)
    walk[::per_track] = 0.0
    pos = np.cumsum(walk, axis=0)
    pos -= np.repeat(pos[::per_track], per_track, axis=0)[:n]
    pos += start[ids]
    return pd.DataFrame({"TRACK_ID": ids.astype(np.uint32), "POSITION_T": (np.arange(n) % per_track).astype(np.uint32),
                         "POSITION_X": pos[:, 0], "POSITION_Y": pos[:, 1],
                         "WIDTH": rng.normal(6.0, 0.5, n).astype(np.float32).astype(np.float64),
                         "HEIGHT": rng.normal(2.0, 0.2, n).astype(np.float32).astype(np.float64),
                         "DEGREES_ANGLE": rng.uniform(-90, 0, n).astype(np.float32).astype(np.float64)}), int(quiet.sum())


def spread(name, values, unit=1e3):
    print("{:<58s} median {:9.2f} ms   min {:9.2f}   max {:9.2f}   ({} rounds)".format(
        name, unit * statistics.median(values), unit * min(values), unit * max(values), len(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--still", type=float, default=0.25, help="share of stationary tracks")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import logging
    import torch
    from ysmr_amd import _lib
    from ysmr_amd import helper_file as hf
    from ysmr_amd.evaluate import evaluate_tracks
    from ysmr_amd.select import select_tracks
    logging.getLogger("ysmr").setLevel(logging.ERROR)
    rng = np.random.default_rng(1)
    dev = torch.device(args.device)
    L = _lib.lib()
    print("device: {}; pandas {}".format(torch.cuda.get_device_name(dev), __import__("pandas").__version__))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def wide_of(df):
        total = 0
        for c in df.columns:
            if df[c].dtype == np.float64:
                a = np.abs(df[c].to_numpy())
                total += int((np.isfinite(a) & (a != 0) & ((a < 2.0 ** -20) | (a >= 2.0 ** 24))).sum())
        return total

    with tempfile.TemporaryDirectory() as folder:
        settings = hf.default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                                          "minimal length in seconds": 20.0, "limit track length to x seconds": 20.0,
                                          "store processed .csv file": True, "store generated statistical .csv file": False,
                                          "store final analysed .csv file": True, "save large plots": False, "save rose plot": False,
                                          "save angle distribution plot / bins": 0, "frame height": 922, "frame width": 1228})
        listed, n_quiet = make_list(args.rows, rng, args.still)
        selected = listed.copy()
        selected.insert(0, "index", np.arange(len(listed), dtype=np.int64))
        selected_csv = os.path.join(folder, "bench_selected_data.csv")
        assert hf.write_table_device(selected.drop(columns="index"), selected_csv, dev) == "device"
        analysed = evaluate_tracks(selected_csv, folder, settings=dict(settings, **{"store final analysed .csv file": False}), fps=30.0,
                                   device=args.device)[0]
        print("{} rows, {} of {} tracks stationary; wide cells: selected table {}, analysed table {} (tp_of_tracks NaN in {} rows)".format(
            args.rows, n_quiet, args.rows // 1000, wide_of(selected), wide_of(analysed), int(analysed["tp_of_tracks"].isna().sum())))
        # ---- the two writers on the same tables ----
        for name, table in (("selected", selected), ("analysed", analysed)):
            a, b = os.path.join(folder, name + "_pandas.csv"), os.path.join(folder, name + "_device.csv")
            hf.save_df_to_csv(table, a, rename_old_file=False)
            assert hf.write_table_device(table, b, dev, rename_old_file=False) == "device"
            size = os.path.getsize(a)
            print("{} shape: {} columns, {} bytes ({:.1f} per row); the two files are the same bytes: {}".format(
                name, table.shape[1], size, size / len(table), open(a, "rb").read() == open(b, "rb").read()))
            host, device, steps = [], [], []
            for r in range(args.rounds):
                host.append(timed(lambda: hf.save_df_to_csv(table, a, rename_old_file=False))[0])
                device.append(timed(lambda: hf.write_table_device(table, b, dev, rename_old_file=False))[0])
                m = dict(hf.LAST_TABLE_WRITE_MARKS)
                steps.append({"upload": m["upload"], "device call": m["format"] - m["upload"], "download": m["download"] - m["format"],
                              "file write": m["written"] - m["download"]})
                print("round {}: {} save_df_to_csv {:9.2f} ms   write_table_device {:9.2f} ms".format(r, name, 1e3 * host[-1], 1e3 * device[-1]))
            spread(name + ": save_df_to_csv (DataFrame.to_csv)", host)
            spread(name + ": write_table_device", device)
            for k in ("upload", "device call", "download", "file write"):
                spread("  " + name + " device step: " + k, [s[k] for s in steps])
            # the device call alone, between two events, columns resident
            plan = hf.table_csv_plan(table)
            tensors = [torch.from_numpy(np.ascontiguousarray(table.iloc[:, k].to_numpy()).view(np.int32) if plan[1][k] == np.uint32
                                        else np.ascontiguousarray(table.iloc[:, k].to_numpy())).to(dev) for k in range(table.shape[1])]
            cols = hf._table_columns([t.data_ptr() for t in tensors], plan[1])
            n = len(table)
            cap, ws_bytes = L.ysmr_table_csv_bound(n, len(plan[1]), cols, len(plan[0])), L.ysmr_table_format_workspace_bytes(n, len(plan[1]), cols)
            ws, csv = torch.empty(ws_bytes, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
            meta = torch.zeros(2, dtype=torch.int64, device=dev)
            kernel_ms = []
            for r in range(args.rounds + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.ysmr_table_format_device(_lib.stream_ptr(dev), n, len(plan[1]), cols, plan[0], len(plan[0]), ws.data_ptr(), ws_bytes,
                                                      csv.data_ptr(), cap, meta.data_ptr(), meta[1:].data_ptr()), "ysmr_table_format_device")
                e1.record()
                torch.cuda.synchronize()
                kernel_ms.append(e0.elapsed_time(e1))
            floats = sum(dt == np.float64 for dt in plan[1])
            spread("  " + name + ": ysmr_table_format_device, device time", kernel_ms[1:], unit=1.0)
            print("  ... {:.2f} ns per row, {:.2f} ns per float64 field ({} per row, {} wide cells), workspace {:.0f} MB".format(
                1e6 * statistics.median(kernel_ms[1:]) / n, 1e6 * statistics.median(kernel_ms[1:]) / (n * floats), floats, int(meta[1]),
                ws_bytes / 1e6))
            del tensors, ws, csv
        # ---- the yardstick: the list's formatter on the same number of rows ----
        rows = np.zeros(args.rows, _lib.ROW_DTYPE)
        rows["track_id"], rows["frame"] = listed["TRACK_ID"], listed["POSITION_T"]
        rows["x"], rows["y"] = listed["POSITION_X"], listed["POSITION_Y"]          # (positions: all in range for its printer)
        rows["w"], rows["h"], rows["angle"] = listed["WIDTH"], listed["HEIGHT"], listed["DEGREES_ANGLE"]
        rows_dev = torch.from_numpy(rows.view(np.uint8)).to(dev)
        n = args.rows
        for via_pandas in (0, 1):
            cap, ws_bytes = L.ysmr_rows_csv_bound(n, 1), L.ysmr_rows_format_device_workspace_bytes(n)
            ws, csv = torch.empty(ws_bytes, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
            colbuf, meta = torch.empty(48 * n, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
            base, kernel_ms = colbuf.data_ptr(), []
            for r in range(args.rounds + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.ysmr_rows_format_device(_lib.stream_ptr(dev), rows_dev.data_ptr(), n, 1, via_pandas, ws.data_ptr(), ws_bytes,
                                                     csv.data_ptr(), cap, meta.data_ptr(), base, base + 4 * n,
                                                     *[base + 8 * n + 8 * n * k for k in range(5)], meta[1:].data_ptr()), "ysmr_rows_format_device")
                e1.record()
                torch.cuda.synchronize()
                kernel_ms.append(e0.elapsed_time(e1))
            spread("yardstick: ysmr_rows_format_device, via_pandas={}, device time".format(via_pandas), kernel_ms[1:], unit=1.0)
            print("  ... {:.2f} ns per row, {:.2f} ns per float64 field (5 per row), unserved rows {}".format(
                1e6 * statistics.median(kernel_ms[1:]) / n, 1e6 * statistics.median(kernel_ms[1:]) / (5 * n), int(meta[1]) & 0xFFFFFFFF))
            del ws, csv, colbuf
        # ---- select_tracks and evaluate_tracks without and with the key ----
        on = dict(settings, **{"hip write csv on device": True})
        kw = dict(path_to_file=os.path.join(folder, "bench_list.csv"), df=listed, fps=30.0, frame_height=922, frame_width=1228, device=args.device)
        results = {}
        for name, s in (("off", settings), ("on", on)):
            os.makedirs(os.path.join(folder, name), exist_ok=True)
            results[name] = select_tracks(settings=dict(s), results_directory=os.path.join(folder, name), **kw)
        same = results["off"] is not None and results["off"].equals(results["on"]) and \
            open(os.path.join(folder, "off", "bench_list_selected_data.csv"), "rb").read() == \
            open(os.path.join(folder, "on", "bench_list_selected_data.csv"), "rb").read()
        print("select_tracks: {} rows selected; the same frame and file with the key: {}".format(
            None if results["off"] is None else len(results["off"]), same))

        def run_select(s, name):
            for f in os.listdir(os.path.join(folder, name)):
                os.unlink(os.path.join(folder, name, f))
            return select_tracks(settings=dict(s), results_directory=os.path.join(folder, name), **kw)

        def run_evaluate(s, name):
            for f in os.listdir(os.path.join(folder, name)):
                os.unlink(os.path.join(folder, name, f))
            return evaluate_tracks(selected_csv, os.path.join(folder, name), settings=dict(s), fps=30.0, device=args.device)
        e_off, e_on = run_evaluate(settings, "off"), run_evaluate(on, "on")
        print("evaluate_tracks: the same frame with the key: {}; the same analysed file: {}".format(
            e_off[0].equals(e_on[0]), open(os.path.join(folder, "off", "bench_selected_data_analysed.csv"), "rb").read() ==
            open(os.path.join(folder, "on", "bench_selected_data_analysed.csv"), "rb").read()))
        s_off, s_on, v_off, v_on = [], [], [], []
        for r in range(args.rounds):
            s_off.append(timed(lambda: run_select(settings, "off"))[0])
            s_on.append(timed(lambda: run_select(on, "on"))[0])
            v_off.append(timed(lambda: run_evaluate(settings, "off"))[0])
            v_on.append(timed(lambda: run_evaluate(on, "on"))[0])
            print("round {}: select_tracks {:9.2f} / {:9.2f} ms   evaluate_tracks {:9.2f} / {:9.2f} ms   (without / with the key)".format(
                r, 1e3 * s_off[-1], 1e3 * s_on[-1], 1e3 * v_off[-1], 1e3 * v_on[-1]))
        spread("select_tracks(df=...), DataFrame.to_csv", s_off)
        spread("select_tracks(df=...), 'hip write csv on device'", s_on)
        spread("evaluate_tracks(path), DataFrame.to_csv", v_off)
        spread("evaluate_tracks(path), 'hip write csv on device'", v_on)


if __name__ == "__main__":
    main()
