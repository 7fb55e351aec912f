"""The host-only part of the device csv reader (csrc/csv_plan.h: sizes, offsets and what they refuse) and the line parser's
host form (csrc/csv_parse.h) under the host's address and undefined-behaviour sanitizers: a stand-alone program
(tests/csv_plan_check.cc, its own ``main``) compares every workspace part with 128-bit arithmetic over text sizes and row
counts -- the limits of the 32-bit offsets and SIZE_MAX among them -- and parses lines kept in heap blocks of exactly their
size.  The sanitizer run covers this program only: nothing of it is loaded into Python and nothing runs on a GPU.  The
library's own answers are asked for the same sizes (pure host calls)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ysmr_amd", "csrc")


def test_the_plan_and_the_line_parser_under_the_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "csv_plan_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "csv_plan_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.startswith("ok ") and not done.stderr.strip(), done.stdout + done.stderr


def test_the_library_refuses_what_the_plan_refuses():
    from ysmr_amd import _lib
    L = _lib.lib()
    limit = 0x7FFFFF00
    for n in (1, 14, 16384, 16385, 80 << 20, limit):
        total = L.ysmr_csv_workspace_bytes(n)
        assert total > 0 and total % 256 == 0 and total >= n // 8 + 4 * (n // 14), n
    for n in (0, limit + 1, 2 ** 31, 2 ** 32, 2 ** 64 - 1):
        assert L.ysmr_csv_workspace_bytes(n) == 0, n
    assert L.ysmr_csv_order_workspace_bytes(2 ** 31 - 1) > 24 * (2 ** 31 - 1)
    for n in (-1, 0, 2 ** 31):
        assert L.ysmr_csv_order_workspace_bytes(n) == 0, n
