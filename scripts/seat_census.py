#!/usr/bin/env python3
"""How often the batch link could run on fewer track waves (CPU only): the live tracks `n` per frame of a clip from the CPU
oracle, and the policy of k_batch's seat block replayed against them -- a track wave is given up at the head of the first
frame whose `n` fits in fewer waves than hold a track; inside a launch that `n` is stale by the deaths of the frame before,
at the start of a launch it is exact; a registration seats new tracks in the lowest free lanes, so the waves in use grow
to ceil(n / 64) and no further.

    python scripts/seat_census.py [blobs] [frames] [frames per launch]      (bench.py's clip: 500 496 248)

Prints the range of n, the frames with n <= 512, the downward crossings of 512, and per launch the events and the frames
run on k track waves -- under the policy, and with seats never given back inside a launch (the kernel before round 17,
taking the waves at a launch's start as ceil(n / 64): a lower bound, the seats it inherits may lie higher)."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ysmr_oracle as yo
from ysmr_amd.synth import SyntheticVideo

blobs = int(sys.argv[1]) if len(sys.argv) > 1 else 500
n_frames = int(sys.argv[2]) if len(sys.argv) > 2 else 496
per_launch = int(sys.argv[3]) if len(sys.argv) > 3 else 248
H, W = 922, 1228

yo.build()
frames = SyntheticVideo(H, W, blobs, seed=0, fps=30.0).frames(n_frames)
rows, _ = yo.track_frames(frames, fps=30.0)
ids = [set() for _ in range(n_frames)]
for r in rows:
    ids[int(r[0])].add(int(r[1]))
n = np.array([len(s) for s in ids])
deaths = np.array([len(ids[f - 1] - ids[f]) if f else 0 for f in range(n_frames)])
print(f"SyntheticVideo({H}, {W}, {blobs}, seed=0), {n_frames} frames, default settings: live tracks per frame (rows per frame)")
print(f"n: min {n.min()}, max {n.max()}, first frame {n[0]}, last frame {n[-1]}")
for f0 in range(0, n_frames, per_launch):
    s = n[f0:f0 + per_launch]
    print(f"launch of frames {f0} .. {f0 + len(s) - 1}: n <= 512 in {int((s <= 512).sum())} of {len(s)} frames")
print(f"n <= 512 in {int((n <= 512).sum())} of {n_frames} frames; crossings of 512 downward: "
      f"{int(((n[:-1] > 512) & (n[1:] <= 512)).sum())}, upward: {int(((n[:-1] <= 512) & (n[1:] > 512)).sum())}")


def waves(k):
    return (int(k) + 63) >> 6


for name, give_back in (("a track wave is given up as soon as n fits in fewer", True), ("seats are never given back inside a launch", False)):
    print(name + ":")
    total_events, total_hist = 0, collections.Counter()
    for f0 in range(0, n_frames, per_launch):
        w = waves(n[f0 - 1]) if f0 else 0
        events, hist = 0, collections.Counter()
        for f in range(f0, min(f0 + per_launch, n_frames)):
            head = n[f - 1] + (deaths[f - 1] if f > f0 else 0) if f else 0      # stale by the last frame's deaths inside a launch
            if give_back and waves(head) < w:
                w, events = waves(head), events + 1
            hist[w] += 1                                   # the waves the frame's search runs on
            w = max(w, waves(n[f] + deaths[f]))            # a registration seats new tracks (a frame registers or ages, never both)
        print(f"  launch of frames {f0} .. {min(f0 + per_launch, n_frames) - 1}: {events} events; frames on k track waves: {dict(sorted(hist.items()))}")
        total_events += events
        total_hist.update(hist)
    print(f"  clip: {total_events} events; frames on k track waves: {dict(sorted(total_hist.items()))}")
