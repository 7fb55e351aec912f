"""track_bacteria end to end from a Motion-JPEG AVI of the bench clip (S500, 1228 x 922, 1920 frames), decoded on the device
('hip decode mjpeg' 'always', ysmr_mjpeg_decode_batch: files without restart markers too) against the host path (False: Pillow on the feed's reader threads).

  python3 scripts/mjpeg_decode_e2e.py make DIR      # DIR/restart.avi: the project's own encoder at quality 90, 4:4:4, one restart
                                                    # interval per MCU row; DIR/plain.avi: the same frames by Pillow, gray, NO
                                                    # restart markers -- the serial worst case (skipped where Pillow is missing)
  python3 scripts/mjpeg_decode_e2e.py run FILE      # False and True alternate, three warm runs each: frames/s, medians
  python3 scripts/mjpeg_decode_e2e.py batch FILE    # the first batches of FILE through ysmr_mjpeg_decode_batch alone, timed by events;
  python3 scripts/mjpeg_decode_e2e.py batch FILE sync      # ... through ysmr_mjpeg_decode_batch_sync (frames without restart markers
                                                    # are many lanes' work there), where the library has it;
                                                    # under `rocprofv3 --kernel-trace --stats --output-format csv -d OUT --` for ...
  python3 scripts/mjpeg_decode_e2e.py kernels OUT   # ... the k_mjd_* kernels' time per batch
  python3 scripts/mjpeg_decode_e2e.py run FILE device      # the device path alone, one warm run and one more; under
                                                    # `rocprofv3 --kernel-trace --output-format csv -d OUT --` for ...
  python3 scripts/mjpeg_decode_e2e.py cotenancy OUT # ... every launch of the threshold kernel against 1.5 x its median, and
                                                    # whether a decode kernel ran beside the slow ones
  python3 scripts/mjpeg_decode_e2e.py --libs A.so B.so     # the same, and the `batch` step also with other builds of the library
                                                    # (YSMR_HIP_LIB): variants of a kernel measured on the same box in the same run
  python3 scripts/mjpeg_decode_e2e.py               # all of it in a temporary directory: every step a child process under its own
                                                    # time limit, and a step that fails ends the run

The output of the last form belongs in profiles/mjpeg_decode_e2e.log (profiles/mjpeg_decode_sync_e2e.log: the run with --libs and the
parent commit's library, after ysmr_mjpeg_decode_batch_sync was added)."""
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH, BLOBS, FRAMES, QUALITY, BATCH = 922, 1228, 500, 1920, 90, 248


def settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False})
    s.update(kw)
    return s


def make(folder, frames=FRAMES):
    import pandas as pd
    from ysmr_amd import annotate_video
    from ysmr_amd.synth import SyntheticVideo
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from avi_tools import write_avi
    clip = SyntheticVideo(HEIGHT, WIDTH, BLOBS, seed=0).frames(frames)
    np.save(os.path.join(folder, "clip.npy"), clip)
    # the project's encoder writes what annotate_video is given; a table of one row paints one small mark into frame 0
    df = pd.DataFrame({"TRACK_ID": np.zeros(1, np.int64), "POSITION_T": np.zeros(1, np.int64), "POSITION_X": [4.0], "POSITION_Y": [4.0],
                       "moving": np.ones(1, np.int8), "turn_points": np.zeros(1, np.int8), "motility_phenotype": np.zeros(1, np.int8)})
    s = settings(**{"save video file extension": ".avi", "save video fourcc codec": "MJPG", "frames per second": 30.0,
                    "hip video jpeg quality": QUALITY})
    written = annotate_video(os.path.join(folder, "clip.npy"), df, settings=s, result_folder=folder)
    os.replace(written, os.path.join(folder, "restart.avi"))
    print("restart.avi: {} frames, {:.0f} KB per frame".format(frames, os.path.getsize(os.path.join(folder, "restart.avi")) / frames / 1e3))
    try:
        from PIL import Image
    except ImportError as exc:
        print("plain.avi: not written ({})".format(exc))
        return
    import io
    from concurrent.futures import ThreadPoolExecutor

    def one(frame):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, format="JPEG", quality=QUALITY)
        return buf.getvalue()

    with ThreadPoolExecutor(16) as pool:
        blobs = list(pool.map(one, clip))
    write_avi(os.path.join(folder, "plain.avi"), clip, 24, fps=(30, 1), jpeg=blobs)
    print("plain.avi: {} frames, {:.0f} KB per frame".format(frames, os.path.getsize(os.path.join(folder, "plain.avi")) / frames / 1e3))


def run(path, reps=3, modes=(False, True)):
    import torch
    from ysmr_amd.frames import open_video
    from ysmr_amd.track_eval import track_bacteria
    video = open_video(path)
    frames, layout = video.frames_available, video.jpeg_layout_for(BATCH, needs_restart=False)
    video.close()
    out = tempfile.mkdtemp(prefix="mjpeg_decode_e2e_")
    rates, rows = {False: [], True: []}, {}
    try:
        for rep in range(reps + 1):                                  # (the first pair warms up: library, allocator, page cache)
            for on_device in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = track_bacteria(path, settings=settings(**{"hip decode mjpeg": "always" if on_device else False}), result_folder=out)
                dt = time.perf_counter() - t0
                rows[on_device] = len(res[0])
                if rep:
                    rates[on_device].append(frames / dt)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    name = os.path.basename(path)
    print("{}: jpeg_layout {}".format(name, layout))
    for on_device in modes:
        print("{}: 'hip decode mjpeg' {}: {} frames/s, median {:.0f} ({} rows)".format(
            name, on_device, " ".join("{:.0f}".format(r) for r in rates[on_device]), statistics.median(rates[on_device]), rows[on_device]))
    assert len(set(rows.values())) == 1, "the two paths tracked different tables"


def batch(path, repeats=5, sync=False):
    """ysmr_mjpeg_decode_batch (``sync``: ysmr_mjpeg_decode_batch_sync) alone on the first batch of the file: milliseconds per
    batch by events.  A library built before the second entry existed says so and is passed over."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.frames import AviVideo
    video = AviVideo(path)
    sampling, largest, most = video.jpeg_layout_for(BATCH, needs_restart=False)
    n = min(BATCH, video.frames_available)
    host, offsets = np.empty(most, np.uint8), np.zeros(n + 1, np.int64)
    assert video.read_jpeg_into(0, n, host, offsets) == n
    # (the library is bound here, entry by entry: a build from before ysmr_mjpeg_decode_batch_sync, given with --libs, still
    # serves the older entry, and _lib.lib() rightly refuses a library that lacks a function it binds)
    import ctypes
    L = ctypes.CDLL(_lib.LIB_PATH)
    name = "ysmr_mjpeg_decode_batch_sync" if sync else "ysmr_mjpeg_decode_batch"
    if not hasattr(L, name):
        print("{}: {}: not in {}".format(os.path.basename(path), name, _lib.LIB_PATH))
        return
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.ysmr_last_error.restype = ctypes.c_char_p
    L.ysmr_mjpeg_decode_workspace_bytes.argtypes, L.ysmr_mjpeg_decode_workspace_bytes.restype = [ci] * 5, ctypes.c_size_t
    L.ysmr_mjpeg_decode_batch.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp]
    if sync:
        L.ysmr_mjpeg_decode_sync_workspace_bytes.argtypes, L.ysmr_mjpeg_decode_sync_workspace_bytes.restype = [ci] * 6, ctypes.c_size_t
        L.ysmr_mjpeg_decode_batch_sync.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp, vp]

    def check(rc):
        if rc:
            raise RuntimeError("{} failed (code {}): {}".format(name, rc, L.ysmr_last_error().decode("utf-8", "replace")))

    chunks, offsets_dev = torch.from_numpy(host).cuda(), torch.from_numpy(offsets).cuda()
    if sync:
        ws_bytes = L.ysmr_mjpeg_decode_sync_workspace_bytes(n, video.height, video.width, video.channels, sampling, largest)
    else:
        ws_bytes = L.ysmr_mjpeg_decode_workspace_bytes(n, video.height, video.width, video.channels, sampling)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, video.height, video.width, video.channels), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    times = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if sync:
            check(L.ysmr_mjpeg_decode_batch_sync(None, chunks.data_ptr(), offsets_dev.data_ptr(), n, video.height, video.width,
                                                 video.channels, sampling, largest, ws.data_ptr(), ws_bytes, out.data_ptr(),
                                                 status.data_ptr()))
        else:
            check(L.ysmr_mjpeg_decode_batch(None, chunks.data_ptr(), offsets_dev.data_ptr(), n, video.height, video.width, video.channels,
                                            sampling, ws.data_ptr(), ws_bytes, out.data_ptr(), status.data_ptr()))
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    assert not status.any().item(), "a frame was flagged"
    print("{}: {}, {} frames, {:.1f} MB of chunks, workspace {:.0f} MB: {} ms, median {:.2f} ms = {:.0f} frames/s".format(
        os.path.basename(path), name, n, offsets[n] / 1e6, ws_bytes / 1e6, " ".join("{:.2f}".format(t) for t in times[1:]),
        statistics.median(times[1:]), n / statistics.median(times[1:]) * 1e3))
    video.close()


def kernels(folder):
    found = glob.glob(os.path.join(folder, "**", "*_kernel_stats.csv"), recursive=True)
    for row in csv.DictReader(open(max(found, key=os.path.getmtime))):
        if "k_mjd_" in row["Name"]:
            name = row["Name"][row["Name"].index("k_mjd_"):].split("(")[0]
            print("  {:14s} calls {:>3s}  average {:9.1f} us  (min {:.1f}, max {:.1f})".format(
                name[:14], row["Calls"], float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))


def cotenancy(folder):
    found = glob.glob(os.path.join(folder, "**", "*_kernel_trace.csv"), recursive=True)
    launches = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(max(found, key=os.path.getmtime)))]
    decode = [(a, b) for name, a, b in launches if "k_mjd_" in name]
    thr = [(a, b) for name, a, b in launches if "k_threshold" in name]
    med = statistics.median(b - a for a, b in thr)
    slow = [(a, b) for a, b in thr if b - a > 1.5 * med]
    beside = sum(1 for a, b in slow if any(c < b and d > a for c, d in decode))
    shared = sum(1 for a, b in thr if any(c < b and d > a for c, d in decode))
    print("  threshold kernel: {} launches, median {:.1f} us, longest {:.1f} us; {} over 1.5 x the median, {} of them beside a decode "
          "kernel; {} launches in all ran beside one".format(len(thr), med / 1e3, max(b - a for a, b in thr) / 1e3, len(slow), beside, shared))


def everything(libs=()):
    work = tempfile.mkdtemp(prefix="mjpeg_decode_e2e_")
    me = [sys.executable, os.path.abspath(__file__)]
    try:
        steps = [(me + ["make", work], 600)]
        for name in ("restart.avi", "plain.avi"):
            path = os.path.join(work, name)
            steps.append((me + ["run", path], 300))
            steps.append((["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(work, "trace_" + name),
                           "--"] + me + ["batch", path], 300))
            steps.append((me + ["kernels", os.path.join(work, "trace_" + name)], 60))
            # the entry that decodes a frame without restart markers with many lanes: the same batch, then its kernels
            steps.append((me + ["batch", path, "sync"], 300))
            steps.append((["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(work, "sync_" + name),
                           "--"] + me + ["batch", path, "sync"], 300))
            steps.append((me + ["kernels", os.path.join(work, "sync_" + name)], 60))
            for lib in libs:                                           # the same batch through other builds, on the same box
                steps.append((me + ["batch", path], 300, lib))
                steps.append((me + ["batch", path, "sync"], 300, lib))
            steps.append((["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(work, "pipe_" + name), "--"] + me +
                          ["run", path, "device"], 300))
            steps.append((me + ["cotenancy", os.path.join(work, "pipe_" + name)], 60))
        for command, limit, *lib in steps:
            if not os.path.exists(os.path.join(work, "plain.avi")) and any("plain.avi" in part for part in command):
                continue
            env = dict(os.environ, YSMR_HIP_LIB=os.path.abspath(lib[0])) if lib else None
            if lib:
                print("YSMR_HIP_LIB={}:".format(lib[0]), flush=True)
            done = subprocess.run(command, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
            lines = [ln for ln in done.stdout.splitlines() if command[0] != "rocprofv3" or ".avi: " in ln]
            print("\n".join(lines), flush=True)
            if done.returncode != 0:                               # nothing more is started on the device after a failure
                print(done.stdout[-4000:])
                sys.exit("step {} ended with {}".format(" ".join(command[:4]), done.returncode))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) == 1:
        everything()
    elif sys.argv[1] == "--libs":
        everything(sys.argv[2:])
    elif sys.argv[1] == "make":
        make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else FRAMES)
    elif sys.argv[1] == "run":
        if len(sys.argv) > 3 and sys.argv[3] == "device":
            run(sys.argv[2], reps=1, modes=(True,))
        else:
            run(sys.argv[2])
    elif sys.argv[1] == "batch":
        batch(sys.argv[2], sync=len(sys.argv) > 3 and sys.argv[3] == "sync")
    elif sys.argv[1] == "kernels":
        kernels(sys.argv[2])
    elif sys.argv[1] == "cotenancy":
        cotenancy(sys.argv[2])
    else:
        sys.exit(__doc__)
