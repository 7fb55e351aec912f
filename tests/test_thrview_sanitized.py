"""The threshold view's pixel rule on the CPU under the sanitizers: a stand-alone program (tests/thrview_rule_check.cc, its own
``main``) built as plain C++ with the host's address and undefined-behaviour sanitizers around csrc/thrview_rule.h -- the body
of ``ysmr_thrview_batch_host`` and the code that decides a pixel in the kernel.  It goes through the shapes of
tests/thrview_model.py in every mode, with 1 and 3 channels, both row orders and two layouts, every input a heap block of its
exact size and the output between guard bytes; its output is compared with the model's, by hash.  Nothing of it is loaded
into Python, nothing is preloaded and nothing runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import thrview_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ysmr_amd", "csrc")


def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def lcg_bytes(state, count):
    """``count`` bytes of the program's generator from ``state`` on -> (bytes, the state behind them)."""
    out = np.empty(count, np.uint8)
    for i in range(count):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = state >> 24
    return out, state


def test_the_rule_runs_clean_under_the_sanitizers_and_stores_what_the_model_stores(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "thrview_rule_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(HERE, "thrview_rule_check.cc"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr.strip(), done.stdout[-2000:] + done.stderr[-4000:]
    lines = done.stdout.splitlines()
    assert lines[-1] == "ok {}".format(len(T.SHAPES) * 2 * 3 * 2 * 2)
    got = {tuple(int(v) for v in line.split()[1:9]): line.split()[9] for line in lines[:-1]}
    assert len(got) == len(lines) - 1
    inputs = {}
    for (n, h, w, channels, mode, bottom_up, stride, frame_bytes), digest in got.items():
        assert (n, h, w) in T.SHAPES
        if (n, h, w, channels) not in inputs:
            pixels = n * h * w
            frames, state = lcg_bytes(w * 1000 + h * 10 + channels, pixels * channels)
            cls, state = lcg_bytes(state, pixels)
            mask, _ = lcg_bytes(state, pixels)
            inputs[n, h, w, channels] = (frames.reshape((n, h, w) if channels == 1 else (n, h, w, 3)), (cls & 7).reshape(n, h, w),
                                         np.where(mask & 8, 255, 0).astype(np.uint8).reshape(n, h, w))
        frames, cls, mask = inputs[n, h, w, channels]
        want = T.stored(frames, cls, mask, mode, stride, bottom_up, frame_bytes, fill=0xA5)
        assert digest == "{:016x}".format(fnv1a(want.tobytes())), (n, h, w, channels, mode, bottom_up, stride)
    assert len(T.combinations(*inputs[2, 3, 1040, 1][1:])) == 8
