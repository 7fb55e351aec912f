"""The typed csv parse's host-only rules (csrc/csv_plan.h: ``typed_fields_rule``) and its line parser's host form
(csrc/csv_parse.h: ``parse_line_typed``) under the host's address and undefined-behaviour sanitizers: a stand-alone program
(tests/csv_typed_check.cc, its own ``main``) walks field lists at the limits of their rules and parses lines kept in heap
blocks of exactly their size, integers at the ends of their types among them.  The sanitizer run covers this program only:
nothing of it is loaded into Python and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ysmr_amd", "csrc")


def test_the_field_rules_and_the_typed_line_parser_under_the_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "csv_typed_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "csv_typed_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.startswith("ok ") and not done.stderr.strip(), done.stdout + done.stderr
