"""track_bacteria end to end with and without the detection view ('hip save detection video') on the benchmark's kind of clip
(default: 1228 x 922 gray, 500 blobs, 480 frames from ysmr_amd.synth), the three modes alternated in ONE process:

  off    the key absent: the pass as it has always been
  raw    the key on, an uncompressed 24-bit AVI ('save video fourcc codec' = 'DIB ')
  mjpg   the key on, Motion-JPEG at --quality

  python3 scripts/view_e2e.py                    # one warm round, then --repeats rounds in which every mode runs once

Per run: wall time of the track_bacteria call (the csv included), frames/s, the size of the detection video; then the
medians.  Every run's csv is compared with the first 'off' run's, byte for byte.  The output belongs in
profiles/view_e2e.log.  What it does NOT separate: the disk (the uncompressed file is 3.4 MB per frame and --tmp decides
where it goes), and the pass's own serial tail (csv and DataFrame), which all three modes share."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("off", "raw", "mjpg")


def settings_of(args, mode):
    from ysmr_amd.helper_file import default_settings
    more = {}
    if mode != "off":
        more = {"hip save detection video": True, "save video file extension": ".avi",
                "save video fourcc codec": "DIB " if mode == "raw" else "MJPG", "hip video jpeg quality": args.quality}
    return default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                               "set logging level (debug/info/warning/critical)": "warning", "log_level": 30,
                               "minimal frame count": 1, **more})


def main(args):
    import torch
    from ysmr_amd.synth import SyntheticVideo
    from ysmr_amd.track_eval import detection_video_path, track_bacteria
    work = tempfile.mkdtemp(prefix="view_e2e_", dir=args.tmp)
    try:
        clip = os.path.join(work, "clip.npy")
        frames = np.lib.format.open_memmap(clip, mode="w+", dtype=np.uint8, shape=(args.frames, args.height, args.width))
        source = SyntheticVideo(args.height, args.width, args.blobs, seed=0)
        for i in range(args.frames):
            frames[i] = source.next_frame()
        frames.flush()
        del frames
        print("clip: {} frames of {} x {}, {} blobs; quality {}; {} warm round(s), {} measured; free space in {}: {:.1f} GB".format(
            args.frames, args.width, args.height, args.blobs, args.quality, args.warm, args.repeats, work,
            shutil.disk_usage(work).free / 1e9), flush=True)
        results = {m: [] for m in MODES}
        reference = None
        for rnd in range(args.warm + args.repeats):
            for mode in MODES:
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
                video = detection_video_path(clip, out_dir, s)
                assert os.path.isfile(video) == (mode != "off")
                size = os.path.getsize(video) if mode != "off" else 0
                shutil.rmtree(out_dir, ignore_errors=True)
                line = "{:<5}: {:8.3f} s  {:8.1f} frames/s  {:7.1f} MB of video ({} rows)".format(mode, dt, args.frames / dt, size / 1e6, len(got[0]))
                if rnd < args.warm:
                    print("  warm     " + line, flush=True)
                else:
                    print("  round {:<2} ".format(rnd - args.warm + 1) + line, flush=True)
                    results[mode].append(args.frames / dt)
        print("medians of the {} measured rounds (frames/s: min .. max); every csv equal to the first:".format(args.repeats))
        for mode in MODES:
            fps = sorted(results[mode])
            print("  {:<5}: {:8.1f} frames/s ({:.1f} .. {:.1f})".format(mode, float(np.median(fps)), fps[0], fps[-1]))
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
    ap.add_argument("--tmp", default=None, help="where the clip and the output go (removed afterwards)")
    main(ap.parse_args())
