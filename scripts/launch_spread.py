"""Per-launch durations of k_bgrid and k_batch in a rocprofv3 --kernel-trace csv (the last 40 launches: bench.py's timed steps):
mean, median, extremes and standard deviation -- the run-to-run spread a change of either is held against.
usage: launch_spread.py <trace directory>"""
import csv, glob, sys
import numpy as np
for name in ("k_bgrid", "k_batch"):
    d = []
    for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if name + "(" in r["Kernel_Name"]:
                d.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    d = np.array([x for _, x in sorted(d)][-40:])       # the timed steps' launches
    print(f"{name} per launch, last {len(d)} launches: mean {d.mean():.1f} us, p50 {np.median(d):.1f}, min {d.min():.1f}, max {d.max():.1f}, std {d.std():.1f}")
