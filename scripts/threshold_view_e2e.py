"""track_bacteria end to end with and without the threshold view ('hip save threshold video') on the benchmark's kind of clip
(default: 1228 x 922 gray, 500 blobs, 480 frames from ysmr_amd.synth), the modes alternated in ONE process:

  off      the key absent: the pass as it has always been
  mask     the key True, an uncompressed 24-bit AVI ('save video fourcc codec' = 'DIB ')
  markers  'markers', uncompressed
  classes  'classes', uncompressed (the one mode that reads the frames)
  mjpg     'mask' as Motion-JPEG at --quality

  python3 scripts/threshold_view_e2e.py                 # one warm round, then --repeats rounds in which every mode runs once
  python3 scripts/threshold_view_e2e.py --modes off --tree <a checkout of another commit, built>     # for A/B runs of the off path

Per run: wall time of the track_bacteria call (the csv included), frames/s, the size of the threshold video; then the
medians.  Every run's csv is compared with the first run's, byte for byte.  Then, unless --no-kernel: the kernel's own time
for one batch of the clip's real maps, between HIP events, per mode.  The output belongs in profiles/threshold_view_e2e.log.
What it does NOT separate: the disk (the uncompressed file is 3.4 MB per frame and --tmp decides where it goes), and the
pass's own serial tail (csv and DataFrame), which all modes share."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

MODES = ("off", "mask", "markers", "classes", "mjpg")


def settings_of(args, mode):
    from ysmr_amd.helper_file import default_settings
    more = {}
    if mode != "off":
        more = {"hip save threshold video": {"mask": True, "mjpg": "mask"}.get(mode, mode), "save video file extension": ".avi",
                "save video fourcc codec": "MJPG" if mode == "mjpg" else "DIB ", "hip video jpeg quality": args.quality}
    return default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                               "set logging level (debug/info/warning/critical)": "warning", "log_level": 30,
                               "minimal frame count": 1, **more})


def kernel_times(args, clip):
    """ysmr_thrview_batch alone on one batch of the clip's own maps: HIP events around --kernel-repeats launches per mode."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.detect import Detector, threshold_params
    frames = np.load(clip, mmap_mode="r")
    n = min(args.kernel_batch, len(frames))
    h, w = frames.shape[1:3]
    dev = torch.device("cuda:0")
    det = Detector(n, h, w, params=threshold_params(True, 5, 2.0))
    on_dev = torch.from_numpy(np.array(frames[:n])).to(dev)
    res = det.detect(on_dev)
    stride = (3 * w + 3) & ~3
    out = torch.empty((n, stride * h + 8), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    print("the kernel alone, {} frames of {} x {} per launch (their maps as the detector left them), {} launches per mode:".format(
        n, w, h, args.kernel_repeats))
    for mode, name in enumerate(("mask", "markers", "classes")):
        times = []
        for k in range(args.kernel_repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.ysmr_thrview_batch(_lib.stream_ptr(dev), on_dev.data_ptr() if mode == 2 else None, res.cls.data_ptr(),
                                            None if mode == 1 else res.mask.data_ptr(), n, h, w, 1, mode, out.data_ptr() + 8, stride,
                                            stride * h + 8, 1), "ysmr_thrview_batch")
            e1.record()
            torch.cuda.synchronize(dev)
            if k >= 2:
                times.append(e0.elapsed_time(e1) * 1e3)
        read = n * h * w * (1 if mode != 2 else 3)
        moved = read + n * h * stride
        med = float(np.median(times))
        print("  {:<8}: {:8.1f} us median ({:.1f} .. {:.1f}), {:.2f} us per frame, {:.0f} GB/s of the {:.1f} MB read and written".format(
            name, med, min(times), max(times), med / n, moved / med / 1e3, moved / 1e6), flush=True)


def main(args):
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.synth import SyntheticVideo
    from ysmr_amd.track_eval import track_bacteria
    work = tempfile.mkdtemp(prefix="threshold_view_e2e_", dir=args.tmp)
    try:
        clip = args.clip or os.path.join(work, "clip.npy")
        if not os.path.isfile(clip):
            frames = np.lib.format.open_memmap(clip, mode="w+", dtype=np.uint8, shape=(args.frames, args.height, args.width))
            source = SyntheticVideo(args.height, args.width, args.blobs, seed=0)
            for i in range(args.frames):
                frames[i] = source.next_frame()
            frames.flush()
            del frames
        n_frames = len(np.load(clip, mmap_mode="r"))
        name = os.path.splitext(os.path.basename(clip))[0]
        print("library {}; clip: {} frames of {} x {}, {} blobs; quality {}; {} warm round(s), {} measured; free space in {}: {:.1f} GB".format(
            _lib.LIB_PATH, n_frames, args.width, args.height, args.blobs, args.quality, args.warm, args.repeats, work,
            shutil.disk_usage(work).free / 1e9), flush=True)
        results = {m: [] for m in args.modes}
        reference = None
        for rnd in range(args.warm + args.repeats):
            for mode in args.modes:
                out_dir = os.path.join(work, "out")
                os.makedirs(out_dir)
                s = settings_of(args, mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = track_bacteria(clip, settings=s, result_folder=out_dir)
                dt = time.perf_counter() - t0
                assert got is not None
                csv = open(got[4], "rb").read()
                reference = csv if reference is None else reference
                assert csv == reference, "the csv of a '{}' run differs from the first run's".format(mode)
                video = os.path.join(out_dir, name + "_threshold_output.avi")
                assert os.path.isfile(video) == (mode != "off")
                size = os.path.getsize(video) if mode != "off" else 0
                shutil.rmtree(out_dir, ignore_errors=True)
                line = "{:<8}: {:8.3f} s  {:8.1f} frames/s  {:7.1f} MB of video ({} rows)".format(mode, dt, n_frames / dt, size / 1e6, len(got[0]))
                if rnd < args.warm:
                    print("  warm     " + line, flush=True)
                else:
                    print("  round {:<2} ".format(rnd - args.warm + 1) + line, flush=True)
                    results[mode].append(n_frames / dt)
        print("medians of the {} measured rounds (frames/s: min .. max); every csv equal to the first:".format(args.repeats))
        for mode in args.modes:
            fps = sorted(results[mode])
            print("  {:<8}: {:8.1f} frames/s ({:.1f} .. {:.1f})".format(mode, float(np.median(fps)), fps[0], fps[-1]))
        if not args.no_kernel:
            kernel_times(args, clip)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--height", type=int, default=922)
    ap.add_argument("--width", type=int, default=1228)
    ap.add_argument("--quality", type=int, default=90, help="'hip video jpeg quality' of the mjpg mode")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--clip", default=None, help="a .npy clip to use (made here if it does not exist) instead of a temporary one")
    ap.add_argument("--tree", default=None, help="import ysmr_amd from this checkout (another commit's, built) instead of this one")
    ap.add_argument("--no-kernel", action="store_true", help="skip the timing of the kernel alone")
    ap.add_argument("--kernel-batch", type=int, default=64)
    ap.add_argument("--kernel-repeats", type=int, default=20)
    ap.add_argument("--tmp", default=None, help="where the clip and the output go (removed afterwards)")
    parsed = ap.parse_args()
    sys.path.insert(0, os.path.abspath(parsed.tree) if parsed.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(parsed)
