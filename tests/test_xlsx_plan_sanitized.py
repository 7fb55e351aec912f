"""The host-only part of the worksheet printer (csrc/xlsx_plan.h: the longest row, the bound, the workspace and what they
refuse) and the row printer's host form (csrc/xlsx_row.h) under the host's address and undefined-behaviour sanitizers: a
stand-alone program (tests/xlsx_plan_check.cc, its own ``main``) compares the sizes with 128-bit arithmetic up to the refused
limits and prints rows into heap blocks of exactly the plan's row size.  The sanitizer run covers this program only: nothing of
it is loaded into Python and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ysmr_amd", "csrc")


def test_the_sheet_plan_and_the_row_printer_under_the_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "xlsx_plan_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "xlsx_plan_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.startswith("ok ") and not done.stderr.strip(), done.stdout + done.stderr
