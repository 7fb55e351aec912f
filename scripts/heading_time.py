"""Time the two calls that take a heading -- evaluate_columns and device_angle_histogram -- on the at-scale table of
tests/test_gpu_tables_at_scale.py (make_table(21, n_tracks=1500, max_len=260), tracks of >= 32 rows; fps 29.97; the histogram at
lag 5 and 36 bins).  One process times one library: run it once per build (YSMR_HIP_LIB=<libysmr_hip.so>), alternating, and
compare the JSON lines (profiles/heading_atan2_ab.log).  Per call: wall clock with a device synchronise, median and minimum.
usage: [YSMR_HIP_LIB=...] python scripts/heading_time.py [--reps 15]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    import torch
    from select_tables import make_table, select_settings
    from ysmr_amd.evaluate import evaluate_columns, evaluate_params
    from ysmr_amd.plot_functions import device_angle_histogram
    df = make_table(21, n_tracks=1500, max_len=260)
    df = df[df.groupby("TRACK_ID")["TRACK_ID"].transform("size") >= 32].reset_index(drop=True)
    p = evaluate_params(select_settings(), 29.97)

    def timed(f, reps):
        f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3), float(np.min(ts) * 1e3)

    rows, stats = evaluate_columns(df, p)
    ev = timed(lambda: evaluate_columns(df, p), args.reps)
    dev = "cuda:0"
    ids = torch.from_numpy(df["TRACK_ID"].to_numpy().astype(np.uint32).view(np.int32)).to(dev)
    x, y = (torch.from_numpy(df[c].to_numpy()).to(dev) for c in ("POSITION_X", "POSITION_Y"))
    moving = torch.from_numpy(np.ascontiguousarray(rows["moving"], dtype=np.int8)).to(dev)
    edges = np.linspace(-np.pi, np.pi, 37)
    counts, points = device_angle_histogram(ids, x, y, moving, 5, edges, dev)
    hist = timed(lambda: device_angle_histogram(ids, x, y, moving, 5, edges, dev), 2 * args.reps)
    print(json.dumps({"lib": os.environ.get("YSMR_HIP_LIB", "default"), "rows": len(df), "tracks": int(stats.shape[0]),
                      "evaluate_columns_ms_median": ev[0], "evaluate_columns_ms_min": ev[1],
                      "angle_histogram_ms_median": hist[0], "angle_histogram_ms_min": hist[1],
                      "angle_diff_sum": int(np.asarray(rows["angle_diff"]).sum()), "hist_sum": int(counts.sum()), "points": points}),
          flush=True)


if __name__ == "__main__":
    main()
