"""annotate_video end to end on a synthetic clip (default 1228 x 922 gray, 400 frames, 500 marks per frame), and the
kernel / copy times of a traced run of the same.

  python3 scripts/annotate_e2e.py                      # frames/s end to end (one warm-up on a tiny clip first)
  python3 scripts/annotate_e2e.py --codec MJPG --quality 90      # the same as Motion-JPEG (default: --codec 'DIB ')
  python3 scripts/annotate_e2e.py --codec MJPG --subsampling 4:2:0 --huffman optimised      # ... subsampled, tables per frame
  python3 scripts/annotate_e2e.py --scene --ab --repeats 5       # Motion-JPEG: 4:4:4, 4:2:2, 4:2:0, each with standard and
                                                                 # optimised tables, alternated on ONE clip in one process:
                                                                 # bytes per frame, frames/s and the encode call's time per
                                                                 # batch (device events) of every run, then the medians
  rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- python3 scripts/annotate_e2e.py
  python3 scripts/annotate_e2e.py --parse DIR          # annotate kernels and device-to-host copies per batch, their ratio

The output of the three, in that order, belongs in profiles/annotate_e2e.log (profiles/mjpeg_e2e.log for Motion-JPEG); that
of --ab in profiles/mjpeg_sampling_e2e.log."""
import argparse
import csv
import glob
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table(n_frames, tracks, height, width, seed=0):
    import pandas as pd
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(0, width, tracks), rng.uniform(0, height, tracks)
    vx, vy = rng.uniform(-1, 1, tracks), rng.uniform(-1, 1, tracks)
    t = np.tile(np.arange(n_frames), tracks)
    tid = np.repeat(np.arange(tracks), n_frames)
    return pd.DataFrame({"TRACK_ID": tid.astype(np.int64), "POSITION_T": t.astype(np.int64),
                         "POSITION_X": x0[tid] + vx[tid] * t, "POSITION_Y": y0[tid] + vy[tid] * t,
                         "moving": (rng.random(len(t)) < 0.7).astype(np.int8),
                         "turn_points": (rng.random(len(t)) < 0.1).astype(np.int8),
                         "motility_phenotype": np.repeat(rng.integers(0, 3, tracks), n_frames).astype(np.int8)})


def scene(rng, height, width):
    """A frame like a microscope's: a noisy gray background and a few hundred bright blobs (noise alone is the worst case of
    any codec and says nothing about a video's size)."""
    frame = rng.normal(90.0, 6.0, (height, width))
    yy, xx = np.mgrid[:height, :width]
    for _ in range(300):
        cy, cx, r = rng.uniform(0, height), rng.uniform(0, width), rng.uniform(2.0, 5.0)
        y0, y1, x0, x1 = int(max(0, cy - 3 * r)), int(min(height, cy + 3 * r)), int(max(0, cx - 3 * r)), int(min(width, cx + 3 * r))
        frame[y0:y1, x0:x1] += 120.0 * np.exp(-((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) / (2 * r * r))
    return np.clip(frame, 0, 255).astype(np.uint8)


def settings_of(args, codec, subsampling, huffman):
    from ysmr_amd.helper_file import default_settings
    more = {}
    if subsampling != "4:4:4" or huffman != "standard":          # (the default mode sets neither key, as a user's file would)
        more = {"hip video jpeg subsampling": subsampling, "hip video jpeg huffman": huffman}
    return default_settings(**{"log to file": False, "save video file extension": ".avi", "save video fourcc codec": codec,
                               "frames per second": 30.0, "hip video jpeg quality": args.quality, **more})


class EncodeTimes:
    """Device events around every ``ysmr_mjpeg_encode_batch`` of the process, recorded on the stream the call is given."""

    def __init__(self):
        from ysmr_amd import _lib
        self.lib, self.inner, self.events = _lib.lib(), _lib.lib().ysmr_mjpeg_encode_batch, []
        self.lib.ysmr_mjpeg_encode_batch = self

    def __call__(self, stream, *rest):
        import torch
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        where = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
        start.record(where)
        rc = self.inner(stream, *rest)
        end.record(where)
        self.events.append((start, end))
        return rc

    def take(self):
        """Milliseconds of the calls since the last take (the caller has synchronised)."""
        out, self.events = [a.elapsed_time(b) for a, b in self.events], []
        return out


def ab(args):
    """Six modes alternated on one clip: warm runs first, then ``--repeats`` rounds in which every mode runs once."""
    import torch
    from ysmr_amd import annotate_video
    work = tempfile.mkdtemp(prefix="annotate_e2e_", dir=args.tmp)
    try:
        rng = np.random.default_rng(1)
        clip = os.path.join(work, "clip.npy")
        frames = np.lib.format.open_memmap(clip, mode="w+", dtype=np.uint8, shape=(args.frames, args.height, args.width))
        one = scene(rng, args.height, args.width) if args.scene else rng.integers(0, 255, (args.height, args.width), dtype=np.uint8)
        for i in range(args.frames):
            frames[i] = np.roll(one, i, axis=1)
        frames.flush()
        del frames
        df = table(args.frames, args.tracks, args.height, args.width)
        modes = [(sub, huff) for sub in ("4:4:4", "4:2:2", "4:2:0") for huff in ("standard", "optimised")]
        times = EncodeTimes()
        results = {m: [] for m in modes}
        print("clip: {} frames of {} x {} ({}), {} marks per frame, quality {}; {} warm round(s), {} measured".format(
            args.frames, args.width, args.height, "scene" if args.scene else "noise", args.tracks, args.quality, args.warm, args.repeats))
        for rnd in range(args.warm + args.repeats):
            for mode in modes:
                out_dir = os.path.join(work, "out")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = annotate_video(clip, df, settings=settings_of(args, "MJPG", *mode), result_folder=out_dir)
                dt = time.perf_counter() - t0
                assert out is not None
                torch.cuda.synchronize()
                calls, size = times.take(), os.path.getsize(out)
                shutil.rmtree(out_dir, ignore_errors=True)
                line = "{} {:<9}: {:9.0f} bytes/frame  {:7.1f} frames/s  encode call per batch: mean {:8.3f} ms over {} calls (max {:.3f})".format(
                    *mode, size / args.frames, args.frames / dt, sum(calls) / len(calls), len(calls), max(calls))
                if rnd < args.warm:
                    print("  warm     " + line, flush=True)
                else:
                    print("  round {:<2} ".format(rnd - args.warm + 1) + line, flush=True)
                    results[mode].append((size / args.frames, args.frames / dt, sum(calls) / len(calls)))
        print("medians of the {} measured rounds (frames/s: min .. max):".format(args.repeats))
        for mode in modes:
            r = results[mode]
            fps = sorted(x[1] for x in r)
            print("  {} {:<9}: {:9.0f} bytes/frame  {:7.1f} frames/s ({:.1f} .. {:.1f})  encode call per batch {:8.3f} ms".format(
                *mode, r[0][0], float(np.median(fps)), fps[0], fps[-1], float(np.median([x[2] for x in r]))))
    finally:
        shutil.rmtree(work, ignore_errors=True)


def run(args):
    import torch
    from ysmr_amd import annotate_video
    work = tempfile.mkdtemp(prefix="annotate_e2e_", dir=args.tmp)
    try:
        s = settings_of(args, args.codec, args.subsampling, args.huffman)
        rng = np.random.default_rng(1)
        small = os.path.join(work, "warm.npy")
        np.save(small, rng.integers(0, 255, (8, 64, 64), dtype=np.uint8))
        assert annotate_video(small, table(8, 4, 64, 64), settings=s, result_folder=work) is not None
        clip = os.path.join(work, "clip.npy")
        frames = np.lib.format.open_memmap(clip, mode="w+", dtype=np.uint8, shape=(args.frames, args.height, args.width))
        one = scene(rng, args.height, args.width) if args.scene else rng.integers(0, 255, (args.height, args.width), dtype=np.uint8)
        for i in range(args.frames):
            frames[i] = np.roll(one, i, axis=1)
        frames.flush()
        del frames
        df = table(args.frames, args.tracks, args.height, args.width)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = annotate_video(clip, df, settings=s, result_folder=work)
        dt = time.perf_counter() - t0
        assert out is not None
        size = os.path.getsize(out)
        print("annotate_video [{}{}]: {} frames of {} x {}, {} marks per frame, {:.1f} MB written in {:.3f} s: {:.1f} frames/s, "
              "{:.2f} GB/s to the file, file size {} bytes ({})".format(
                  args.codec.strip(), ", quality {}, {}, {} tables".format(args.quality, args.subsampling, args.huffman)
                  if args.codec.upper() in ("MJPG", "JPEG") else "",
                  args.frames, args.width, args.height, args.tracks, size / 1e6, dt, args.frames / dt, size / dt / 1e9, size, work),
              flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def parse(directory):
    def rows(pattern):
        files = glob.glob(os.path.join(directory, "**", pattern), recursive=True)
        if not files:
            raise SystemExit("no {} under {}".format(pattern, directory))
        return list(csv.DictReader(open(max(files, key=os.path.getmtime))))

    trace = rows("*_kernel_trace.csv")
    kernels = [r for r in trace if "k_pack_dib" in r["Kernel_Name"] or "k_paint_marks" in r["Kernel_Name"]]
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3      # noqa: E731  (us)
    pack = sorted(dur(r) for r in kernels if "k_pack_dib" in r["Kernel_Name"])
    paint = sorted(dur(r) for r in kernels if "k_paint_marks" in r["Kernel_Name"])
    batches = len(pack) - 1                                   # (the first launch is the warm-up clip's)
    moved = rows("*_memory_copy_trace.csv")
    direction = next(k for k in moved[0] if "irection" in k)
    copies = sorted((dur(r) for r in moved if "DEVICE_TO_HOST" in r[direction].upper()), reverse=True)
    copies = copies[:batches]                                 # the batches' copies are the long ones
    pack, paint = pack[1:], paint[1:]
    k_total, c_total = sum(pack) + sum(paint), sum(copies)
    print("traced run: {} batches".format(batches))
    print("  k_pack_dib     per batch: mean {:9.1f} us  (min {:.1f}, max {:.1f})".format(sum(pack) / batches, pack[0], pack[-1]))
    print("  k_paint_marks  per batch: mean {:9.1f} us  (min {:.1f}, max {:.1f})".format(sum(paint) / batches, paint[0], paint[-1]))
    print("  device-to-host per batch: mean {:9.1f} us  (min {:.1f}, max {:.1f})".format(c_total / batches, copies[-1], copies[0]))
    for name in ("k_mj_blocks", "k_mj_blocks_sampled", "k_mj_hist", "k_mj_tables", "k_mj_lengths", "k_mj_pack", "k_mj_count",
                 "k_mj_layout", "k_mj_write"):
        mine = sorted(dur(r) for r in trace if name + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(name))[-batches:] if batches > 0 else []
        if mine:                                                  # (the warm-up clip's launches are the short ones)
            print("  {:<14} per batch: mean {:9.1f} us  (min {:.1f}, max {:.1f})".format(name, sum(mine) / len(mine), mine[0], mine[-1]))
            k_total += sum(mine)
    print("  kernels / copy = {:.4f}  ({})".format(k_total / c_total, "the kernels hide behind the copy" if k_total < c_total
                                                   else "THE KERNELS TAKE LONGER THAN THE COPY"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--tracks", type=int, default=500)
    ap.add_argument("--height", type=int, default=922)
    ap.add_argument("--width", type=int, default=1228)
    ap.add_argument("--codec", default="DIB ", help="'save video fourcc codec': 'DIB ' (uncompressed) or MJPG")
    ap.add_argument("--quality", type=int, default=90, help="'hip video jpeg quality' (Motion-JPEG only)")
    ap.add_argument("--subsampling", default="4:4:4", help="'hip video jpeg subsampling': 4:4:4, 4:2:2 or 4:2:0 (Motion-JPEG only)")
    ap.add_argument("--huffman", default="standard", help="'hip video jpeg huffman': standard or optimised (Motion-JPEG only)")
    ap.add_argument("--ab", action="store_true", help="alternate the six Motion-JPEG modes on one clip")
    ap.add_argument("--repeats", type=int, default=5, help="measured rounds of --ab")
    ap.add_argument("--warm", type=int, default=1, help="rounds of --ab that are run first and not counted")
    ap.add_argument("--scene", action="store_true", help="a microscope-like frame instead of noise")
    ap.add_argument("--tmp", default=None, help="where the clip and the output go (removed afterwards)")
    ap.add_argument("--parse", default=None, help="a rocprofv3 output directory: print the per-batch times")
    a = ap.parse_args()
    parse(a.parse) if a.parse else ab(a) if a.ab else run(a)
