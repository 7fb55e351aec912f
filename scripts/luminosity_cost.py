#!/usr/bin/env python3
"""What 'include luminosity in tracking calculation' costs on the bench clip (recorded, not gated: DESIGN.md 4).

The bench workload (1228 x 922, ~500 blobs, a clip of two batches resident in HBM, detection of batch b+1 beside the link of
batch b) with 'disable gsff' = True, in four forms on one build:

  batch-2d       the default 2-D link (one launch per batch)            -- for orientation
  frame-2d       2-D with ysmr_tracker_link_mode(t, 1): one launch per frame
  lum-3d         luminosity on: k_luminosity behind the labelling chain, ysmr_tracker_run3 as the pipeline runs it (link
                 mode 2: one k_batch3 launch per batch for this shape)
  lum-3d-frame   the same with the handle forced to link mode 1: one launch per frame, what a 3-D handle took before the
                 3-D batch link

    python scripts/luminosity_cost.py [--steps 10] [--warmup 3] [--only lum-3d]

One JSON line per form.  ``--only lum-3d`` under ``rocprofv3 --kernel-trace --stats`` gives k_luminosity's time per batch
beside the labelling chain's, and k_bgrid3 / k_batch3 per batch.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    from ysmr_amd.helper_file import default_settings
    from ysmr_amd.synth import SyntheticVideo
    import ysmr_amd.track_eval as te
    from ysmr_amd.track_eval import TrackingPipeline, auto_batch
    from ysmr_amd.tracker import DeviceTracker

    class PerFrameTracker(DeviceTracker):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.link_mode(1)
    H, W, blobs = 922, 1228, 500
    B = auto_batch(H, W)
    F = 2 * B
    frames = torch.from_numpy(SyntheticVideo(H, W, blobs, seed=0, fps=30.0).frames(F)).cuda()
    for form in ("batch-2d", "frame-2d", "lum-3d", "lum-3d-frame"):
        if args.only and form != args.only:
            continue
        s = default_settings()
        s["disable gsff"] = True
        s["include luminosity in tracking calculation"] = form.startswith("lum-3d")
        # (frame-2d, lum-3d-frame: the handle is told before the detectors are built, so that they take the threshold kernel
        # and the resident grids that go with a per-frame link beside them)
        te.DeviceTracker = PerFrameTracker if form in ("frame-2d", "lum-3d-frame") else DeviceTracker
        pipe = TrackingPipeline(H, W, 30.0, s, batch=B, max_det=2048, capacity=768, rows_per_flush=F * 768)
        te.DeviceTracker = DeviceTracker

        def step():
            pipe.reset()
            pending = None
            for f0 in list(range(0, F, B)) + [None]:
                nxt = (pipe.detect_async(frames[f0:f0 + B], frames_ready=False), f0) if f0 is not None else None
                if pending is not None:
                    (slot, res, ready), p0 = pending
                    pipe.link(slot, res, ready, p0)
                pending = nxt

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n_tracks, next_id, err = pipe.trk.info()
        rows = int(pipe.row_count.item())
        if err or rows <= 0:
            raise SystemExit(f"{form}: tracker error bits {err}, rows {rows}")
        print(json.dumps({"form": form, "frames_per_s": F * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
                          "frames_per_step": F, "batch": B, "rows_per_step": rows, "tracks_alive": n_tracks,
                          "ids_issued": next_id, "batched": pipe.trk.batched, "fused": pipe.trk.fused}), flush=True)
        del pipe


if __name__ == "__main__":
    main()
