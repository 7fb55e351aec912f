"""The detection view's pixel rule on the CPU under the sanitizers: a stand-alone program (tests/view_host_check.cc, its own
``main``) built as plain C++ with the host's address and undefined-behaviour sanitizers around csrc/view_rule.h -- the body of
``ysmr_view_batch_host`` and the code that decides a pixel in the kernels.  It is fed the edge cases of tests/view_model.py
(boxes across every frame edge, wholly outside and with corners at the +-2^20 clamp, ids of ten digits, marks across the
edges, positions that are not finite or beyond int32, rows of other batches) with every buffer at its exact size, and its
output is compared with the model's, by hash and by the numbers of blue and green pixels.  Nothing of it is loaded into
Python and nothing runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import annotate_model as A
import view_model as V

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ysmr_amd", "csrc")
FIRST = 70000


def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def lcg_frames(seed, shape):
    """The frames the program makes for itself from ``seed``."""
    n = int(np.prod(shape))
    state, out = seed, np.empty(n, np.uint8)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = (state >> 24) % 200
    return out.reshape(shape)


def case_text(name, channels, bottom_up, gap, seed, det, det_count, rows, span):
    stride = (3 * V.W + 3) & ~3
    head = "case {} {} {} {} {} {} {} {} {} {} {} {} {} {}".format(name, V.N, V.H, V.W, channels, det.shape[1], len(rows), FIRST, stride,
                                                               stride * V.H + gap, bottom_up, span[0], span[1], seed)
    lines = [head, " ".join(str(int(c)) for c in det_count), " ".join("%.9g" % v for v in det.reshape(-1))]
    lines += ["{} {} {:.17g} {:.17g} {}".format(int(r["frame"]), int(r["track_id"]) & 0xFFFFFFFF, float(r["x"]), float(r["y"]), int(r["disappeared"]))
              for r in rows]
    return "\n".join(lines) + "\n"


def test_the_rule_runs_clean_under_the_sanitizers_and_paints_what_the_model_paints(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "view_host_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(HERE, "view_host_check.cc"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    det, det_count, rows = V.cases(FIRST)
    text, want = "", {}
    for k, (channels, bottom_up, gap) in enumerate(((1, 0, 0), (1, 1, 12), (3, 0, 8), (3, 1, 0))):
        name, seed = "c{}b{}".format(channels, bottom_up), 1234 + k
        text += case_text(name, channels, bottom_up, gap, seed, det, det_count, rows, (0, len(rows)))
        frames = lcg_frames(seed, (V.N, V.H, V.W) if channels == 1 else (V.N, V.H, V.W, 3))
        painted = V.paint(frames, det, det_count, rows, FIRST)
        stride = (3 * V.W + 3) & ~3
        packed = A.pack_dib(painted, bottom_up, stride, stride * V.H + gap, fill=0xA5)
        want[name] = "ok {:016x} {} {}".format(fnv1a(packed.tobytes()), int((painted == (255, 0, 0)).all(axis=3).sum()),
                                               int((painted == (0, 255, 0)).all(axis=3).sum()))
    # the rows as a slice of a longer array, and no rows at all (a NULL pointer)
    frames = lcg_frames(99, (V.N, V.H, V.W))
    text += case_text("slice", 1, 1, 0, 99, det, det_count, rows, (4, len(rows) - 3))
    painted = V.paint(frames, det, det_count, rows[4:len(rows) - 3], FIRST)
    want["slice"] = "ok {:016x} {} {}".format(fnv1a(A.pack_dib(painted, 1, fill=0xA5).tobytes()), int((painted == (255, 0, 0)).all(axis=3).sum()),
                                              int((painted == (0, 255, 0)).all(axis=3).sum()))
    text += case_text("norows", 1, 0, 0, 99, det, det_count, rows[:0], (0, 0))
    painted = V.paint(frames, det, det_count, rows[:0], FIRST)
    want["norows"] = "ok {:016x} {} 0".format(fnv1a(A.pack_dib(painted, 0, fill=0xA5).tobytes()), int((painted == (255, 0, 0)).all(axis=3).sum()))
    done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr.strip(), done.stdout[-2000:] + done.stderr[-4000:]
    got = {}
    for line in done.stdout.splitlines():
        _, name, rest = line.split(" ", 2)
        got[name] = rest
    assert got == want
    assert all(int(v.split()[2]) > 200 for v in want.values()) and int(want["c1b0"].split()[3]) > 200
