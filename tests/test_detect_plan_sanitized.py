"""Detection's host-only part (csrc/detect_plan.h) on the CPU: a stand-alone program (tests/detect_plan_check.cc, its own
``main``) built as plain C++ with the host's address and undefined-behaviour sanitizers.  It is given the rows of
tests/detect_plan_cases.py and prints, per row, what the plan decides -- the geometry check, the workspace's layout, the
threshold kernel with its shape and grid, the labelling chain's grids, the mean-gray branch's, the matrix-pipe kernel's scales
and level constants -- which is compared with the table; and it walks a grid of small shapes through the layout, the strip
kernels' item loops and the matrix-pipe kernel's range cut by itself.  Nothing of it is loaded into Python and nothing runs
on a GPU; the workspace totals are also asked of the library (a pure host call)."""
import os
import shutil
import subprocess

import pytest

import detect_plan_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ysmr_amd", "csrc")


def run_plan_check(tmp_path):
    """The program's output lines, built with the sanitizers and run on the table's rows."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "detect_plan_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(HERE, "detect_plan_check.cc"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    rows = "".join(dc.line_of(*row) + "\n" for row in dc.ROWS)
    done = subprocess.run([exe], input=rows, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and not done.stderr.strip(), done.stdout[-2000:] + done.stderr
    return done.stdout.splitlines()


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    return run_plan_check(tmp_path_factory.mktemp("detect_plan"))


def test_every_row_is_planned_as_the_table_says(plan_lines):
    got = {}
    for line in plan_lines:
        if line.startswith("case "):
            _, name, rest = line.split(" ", 2)
            got[name] = rest
    assert list(got) == [name for _, name, _ in dc.ROWS] == list(dc.EXPECTED)
    for name, expected in dc.EXPECTED.items():
        assert got[name] == expected, name


def test_the_table_has_both_sides_of_the_kernel_choice():
    kernels = {dict(f.split("=", 1) for f in dc.EXPECTED[name].split())["kernel"] for kind, name, _ in dc.ROWS if kind == "thr"}
    assert kernels == {"mfma", "strip", "tile", "refused"}
    errors = {dc.EXPECTED[name] for kind, name, _ in dc.ROWS if kind == "ws" and dc.EXPECTED[name].startswith("error=")}
    assert errors == {"error=positive", "error=channels", "error=too_large"}


def test_layouts_strips_panels_and_scales_hold_over_a_grid_of_shapes(plan_lines):
    walked = [line for line in plan_lines if line.startswith("walk ")]
    assert len(walked) == 1 and walked[0].startswith("walk ok ") and int(walked[0].split()[2]) > 1000, walked


def test_the_library_sizes_the_workspace_as_the_table_says():
    from ysmr_amd import _lib
    lib = _lib.lib()
    asked = 0
    for kind, name, (batch, height, width, _channels, max_det) in (row for row in dc.ROWS if row[0] == "ws"):
        fields = dict(f.split("=", 1) for f in dc.EXPECTED[name].split())
        if "total" in fields:
            assert lib.ysmr_detect_workspace_bytes(batch, height, width, max_det) == int(fields["total"]), name
            asked += 1
        elif fields == {"error": "positive"}:
            assert lib.ysmr_detect_workspace_bytes(batch, height, width, max_det) == 0, name
    assert asked >= 15
