"""The host-only argument and plan code of ``ysmr_tiff_decode_batch`` (csrc/tiff_decode_plan.h) under the host's address and
undefined-behaviour sanitizers: a stand-alone program (tests/tiff_plan_check.cc, its own ``main``) walks a grid of frame counts,
shapes, strip heights and body sizes -- INT_MAX and the first refused values among them -- and compares what is accepted and every
size with 128-bit arithmetic.  Nothing of it is loaded into Python and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ysmr_amd", "csrc")


def test_the_plan_code_under_the_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "plan_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "tiff_plan_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.startswith("ok ") and not done.stderr.strip(), done.stdout + done.stderr
