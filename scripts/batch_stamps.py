"""In-kernel phases of the batch link (k_batch), one frame of a batch, per wave: s_memtime stamps of a stamps build
(scripts/build_stamps.sh; YSMR_HIP_LIB=scripts/var_stamps.so).  usage: batch_stamps.py [blobs] [capacity] [max_det]
The stamped launch is frames 64 .. 127: a build with EXTRA=-DYSMR_BL_FRAME=0 stamps frame 64, which refreshes the window sums
from the ring; its block has a stamp pair of its own and is printed beside that frame and launch frame 40, a steady one."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ysmr_amd import _lib
from ysmr_amd.helper_file import default_settings
from ysmr_amd.synth import SyntheticVideo
from ysmr_amd.track_eval import TrackingPipeline
blobs = int(sys.argv[1]) if len(sys.argv) > 1 else 450
cap = int(sys.argv[2]) if len(sys.argv) > 2 else 512
md = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
F, B, H, W = 128, 64, 922, 1228
frames = torch.from_numpy(SyntheticVideo(H, W, blobs, seed=0).frames(F)).cuda()
pipe = TrackingPipeline(H, W, 30.0, default_settings(), batch=B, max_det=md, capacity=cap, rows_per_flush=F * cap)
res0 = pipe.det[0].detect(frames[:B]); res1 = pipe.det[1].detect(frames[B:]); torch.cuda.synchronize()
L = _lib.lib()
NW = int(os.environ.get("BL_WAVES", "16"))
buf = (ctypes.c_ulonglong * (NW * 16))()
# (a pass of the frame loop: the search and the claim of a frame, barrier A, the ranks and the row of the frame before, the
# rest of the frame; one barrier)
names = ["search + key atomic", "wait (grid block) + barrier A", "dma issue + key read + ranks, row of the frame before",
         "exact claim path", "ageing / deregistration", "registration + clear keys two frames ahead",
         "wait vmcnt(0)", "filter bank"]
# (the stamps in the order a pass meets them: stamp 8 stands behind the frame's wait for vector memory, stamp 7 at the frame's end)
ORDER = [0, 1, 2, 3, 4, 5, 6, 8, 7]
LAST = len(names)
# per wave over the launch's frames (g_bcounts): how often each rarely taken path ran
count_names = ["wave-frames with a lane on the 3 x 3 block search", "lanes on the 3 x 3 block search",
               "wave-frames seeding a new track's filter bank", "wave-frames with a grown filter bank (old track)",
               "frames with registration", "wave-frames refreshing the sums from the ring", "frames with deaths", "deaths",
               "frames on the exact claim path (row of wave 0)"]
acc = []
acc_s = []      # the same stamps of launch frame YSMR_BL_STEADY (g_bsteady)
acc_r = []      # per rep and wave: the refresh block, the stamped frame, launch frame 40 (cycles)
# BESIDE=1: the stamped launch runs while another stream loops over the matrix-pipe threshold kernel on 248 workgroups, as
# in the pipeline (which phase of a frame the memory system's load stretches)
beside = os.environ.get("BESIDE") == "1"
if beside:
    from ysmr_amd.detect import Detector
    side = torch.cuda.Stream()
    det_b = Detector(B, H, W, max_det=md, beside_batch_link=True)
    many = torch.from_numpy(SyntheticVideo(H, W, blobs, seed=1).frames(256)).cuda()
for rep in range(12 if beside else 6):
    pipe.reset()
    pipe.trk.run(res0.det, res0.det_count, 0, pipe.rows, pipe.row_count)
    torch.cuda.synchronize()
    if beside:
        with torch.cuda.stream(side):
            for i in range(8): det_b.threshold(many[(i % 4) * B:(i % 4) * B + B])
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record(); pipe.trk.run(res1.det, res1.det_count, B, pipe.rows, pipe.row_count); t1.record()
    torch.cuda.synchronize()
    if not hasattr(L, "ysmr_debug_read_bstamps"):      # (a plain library: the launch's time without the stamps' own cycles)
        print(f"rep {rep}: launch pair {t0.elapsed_time(t1) * 1e3:.1f} us for {B} frames (no stamps in this library)")
        continue
    L.ysmr_debug_read_bstamps(buf)
    full = np.array(buf[:], dtype=np.int64).reshape(NW, 16)
    a = full[:, ORDER]
    acc.append(a)
    if hasattr(L, "ysmr_debug_read_bsteady"):
        sbuf = (ctypes.c_ulonglong * (NW * 16))()
        L.ysmr_debug_read_bsteady(sbuf)
        acc_s.append(np.array(sbuf[:], dtype=np.int64).reshape(NW, 16)[:, ORDER])
    print("   fast path per wave:", (full[:, 11] - full[:, 0]).tolist(), " lanes left to the wave search:", full[:, 12].tolist())
    print("   over the launch's frames: lanes left to the wave search per wave", full[:, 13].tolist(), "= %.2f per frame; frames in which a wave ran it:" % (full[:, 13].sum() / B), full[:, 14].tolist())
    rt0, rt1, mt0, mt1 = int(full[0, 15]), int(full[1, 15]), int(full[2, 15]), int(full[3, 15])
    if rt1 > rt0:
        print(f"   shader clock over frames 8..56: {(mt1 - mt0) / (rt1 - rt0) * 100:.0f} MHz; {(rt1 - rt0) / 100 / 48:.2f} us and {(mt1 - mt0) / 48:.0f} cycles per frame")
    if hasattr(L, "ysmr_debug_read_bcounts"):
        cnt = (ctypes.c_ulonglong * (NW * len(count_names)))()
        L.ysmr_debug_read_bcounts(cnt)
        cn = np.array(cnt[:], dtype=np.int64).reshape(NW, len(count_names))
        for k, what in enumerate(count_names):
            print(f"   {what:58s}", cn[:, k].tolist())
    if hasattr(L, "ysmr_debug_read_bwaves"):
        hist = (ctypes.c_ulonglong * 17)()
        L.ysmr_debug_read_bwaves(hist)
        print("   frames run on k track waves:", {k: int(v) for k, v in enumerate(hist[:]) if v})
    if hasattr(L, "ysmr_debug_read_bseats"):
        seats = (ctypes.c_ulonglong * 2)()
        L.ysmr_debug_read_bseats(seats)
        print(f"   frames that gave up track waves: {int(seats[0])}, tracks moved in them: {int(seats[1])}")
    if hasattr(L, "ysmr_debug_read_brefresh"):
        # (a build with -DYSMR_BL_FRAME=0 stamps the stamped launch's first frame, frame 64: the one that refreshes)
        rf = (ctypes.c_ulonglong * (NW * 4))()
        L.ysmr_debug_read_brefresh(rf)
        r = np.array(rf[:], dtype=np.int64).reshape(NW, 4)
        acc_r.append(np.stack([r[:, 1] - r[:, 0], a[:, LAST] - a[:, 0], r[:, 3] - r[:, 2]], axis=1))
        print("   refresh block per wave:", acc_r[-1][:, 0].tolist(), " its frame:", acc_r[-1][:, 1].tolist(),
              " steady frame 40:", acc_r[-1][:, 2].tolist())
    print(f"rep {rep}: launch pair {t0.elapsed_time(t1) * 1e3:.1f} us for {B} frames; frame (wave 0) {a[0, LAST] - a[0, 0]} cycles")
for title, stamps in (("the stamped frame (YSMR_BL_FRAME)", acc), ("the steady frame (YSMR_BL_STEADY)", acc_s)):
    if not stamps:
        continue
    a = np.mean(np.array(stamps), axis=0) if beside else np.median(np.array(stamps), axis=0)
    d = np.diff(a, axis=1)
    print(title)
    print("%-44s" % "phase (cycles of s_memtime, 100 MHz? no: shader clock)", " ".join(f"w{w:<6d}" for w in range(NW)))
    for k, n in enumerate(names):
        print("%-44s" % n, " ".join(f"{d[w, k]:<7.0f}" for w in range(NW)))
    print("%-44s" % "frame", " ".join(f"{a[w, LAST] - a[w, 0]:<7.0f}" for w in range(NW)))
    # the exposed wait of the track waves (a wave without a track passes it at once), every rep: the range
    ws = np.array(stamps)[:, :, 7] - np.array(stamps)[:, :, 6]
    print("%-44s" % "wait vmcnt(0), min .. max over the reps", " ".join(f"{ws[:, w].min()}..{ws[:, w].max()}" for w in range(NW)))
if acc_r:
    rr = np.array(acc_r)
    for how, fn in (("median", np.median), ("mean", np.mean), ("max", np.max)):
        v = fn(rr, axis=0)
        for k, n in enumerate(["refresh block", "stamped frame (the refresh's)", "steady frame (launch frame 40)"]):
            print("%-44s" % f"{n}, {how}", " ".join(f"{v[w, k]:<7.0f}" for w in range(NW)))
    # the frame ends for the workgroup where its slowest wave does: what a refresh adds to a frame's critical path
    print("slowest wave per rep: refresh block", rr[:, :, 0].max(axis=1).tolist(), " refresh frame", rr[:, :, 1].max(axis=1).tolist(),
          " steady frame", rr[:, :, 2].max(axis=1).tolist())
print(pipe.trk.info())
