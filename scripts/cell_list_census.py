#!/usr/bin/env python3
"""Which cells of the bench's frames overflow their candidate list, and who pays for it (no GPU needed).

    python scripts/cell_list_census.py [frames=128] [first=64] [blobs=500]

The oracle's detections of SyntheticVideo(922, 1228, blobs, seed=0) go through the oracle's tracker; every frame from
`first` on is binned and listed by tests/cell_list_model.py (the float32 statement of k_bgrid), and every prediction is
placed as bl_search places it.  Reported: crowded cells (flagged 0xFFFF before the split lists) per frame, what they
gather and keep, and of the lanes that take the 3 x 3 block search how many are outside the grid, how many the four
quadrant lists serve, and how many a single list of 16 would serve."""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cell_list_model as M                      # noqa: E402
from oracle import ysmr_oracle as yo             # noqa: E402
from ysmr_amd.synth import SyntheticVideo        # noqa: E402


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    blobs = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    fps = 30.0
    frames = SyntheticVideo(922, 1228, blobs, seed=0).frames(n_frames)
    inv, t_low, t_high, use_high = yo.threshold_params(True, 5, 2.0)
    ot = yo.OracleTracker(max_disappeared=fps, fps=fps, n_min=0, n_max=30, n_f=3)
    per_frame = collections.Counter()
    kept_hist, gathered_hist, quad_kept = collections.Counter(), collections.Counter(), collections.Counter()
    lanes = collections.Counter()
    n_counted = 0
    for f in range(n_frames):
        det = yo.detect_frame(frames[f], inv, t_low, t_high, use_high, 2048).det
        pred = np.array([t.pos for t in ot.tracks], float).reshape(-1, 2)
        if f >= first and len(det) and M.has_lists(len(det)):
            n_counted += 1
            g, order = M.bin_frame(det[:, :2])
            xy = np.asarray(det[:, :2], np.float32)[order]
            detail = {}
            lists, _ = M.frame_lists(g, xy, detail=detail)
            per_frame[len(detail)] += 1
            rank = {c: k for k, c in enumerate(sorted(detail))}
            for c, (kept, n, quads) in detail.items():
                kept_hist["> 32 gathered" if kept is None else len(kept)] += 1
                gathered_hist[min(n, 33)] += 1
                for qk in quads:
                    quad_kept["flagged" if M.flagged(qk) else len(qk)] += 1
            lanes["tracks"] += len(pred)
            for px, py in pred:
                cx, cy, q = M.lane_cell(g, px, py)
                if not (0 <= cx < g.G and 0 <= cy < g.G):
                    lanes["outside the grid"] += 1
                    continue
                c = cy * g.G + cx
                if c not in detail:
                    continue
                kept, n, quads = detail[c]
                lanes["in a crowded cell"] += 1
                lanes["served by quadrant lists"] += not any(M.flagged(qk) for qk in quads)
                lanes["served by quadrant lists, first BL_OVF cells"] += not any(M.flagged(qk) for qk in quads) and rank[c] < M.BL_OVF
                lanes["own quadrant fits (per-quadrant flag)"] += not M.flagged(quads[q])
                lanes["served by a list of 16"] += kept is not None and len(kept) <= 16
        rects = yo.det_to_rects(det)
        ot.update(rects)
    print(f"{n_counted} frames ({first}..{n_frames - 1}), {blobs} blobs, BL_LIST {M.BL_LIST}, BG_CAND {M.BG_CAND}, BL_OVF {M.BL_OVF}")
    print("crowded cells per frame: frames", dict(sorted(per_frame.items())),
          "mean %.2f" % (sum(k * v for k, v in per_frame.items()) / max(n_counted, 1)))
    print("candidates a crowded cell keeps: cells", dict(sorted(kept_hist.items(), key=lambda kv: str(kv[0]).rjust(20))))
    print("candidates a crowded cell gathers (33: more than 32): cells", dict(sorted(gathered_hist.items())))
    print("candidates a quadrant of a crowded cell keeps: quadrants", dict(sorted(quad_kept.items(), key=lambda kv: str(kv[0]).rjust(20))))
    block = lanes["outside the grid"] + lanes["in a crowded cell"]
    print(f"lane-frames: {lanes['tracks']} ({lanes['tracks'] / max(n_counted, 1):.0f} per frame); on the 3 x 3 block search {block} "
          f"({block / max(n_counted, 1):.2f} per frame)")
    for k in ("outside the grid", "in a crowded cell", "served by quadrant lists", "served by quadrant lists, first BL_OVF cells",
              "own quadrant fits (per-quadrant flag)", "served by a list of 16"):
        print(f"  {k:46s} {lanes[k]:6d}  {100.0 * lanes[k] / max(block, 1):5.1f} % of the block's lane-frames")


if __name__ == "__main__":
    main()
