"""The tracker's host-only part (csrc/tracker_plan.h) on the CPU: a stand-alone program (tests/tracker_plan_check.cc, its own
``main``) built as plain C++ with the host's address and undefined-behaviour sanitizers.  It is given the cases of
tests/tracker_plan_cases.py and prints, per case, the link path, the capabilities, the LDS sizes and the state block's total,
which are compared with the table; it walks a grid of shapes through the carving of the state block by itself; and it prints
the batch link's block layout for every detection count, which tests/test_cell_list_model.py compares with its model.
Nothing of it is loaded into Python and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

import tracker_plan_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ysmr_amd", "csrc")


def run_plan_check(tmp_path):
    """The program's output lines, built with the sanitizers and run on the table's cases."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "tracker_plan_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "tracker_plan_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    cases = "".join(tc.line_of(name, changes) + "\n" for name, changes, *_ in tc.CASES)
    done = subprocess.run([exe], input=cases, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and not done.stderr.strip(), done.stdout[-2000:] + done.stderr
    return done.stdout.splitlines()


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    return run_plan_check(tmp_path_factory.mktemp("plan"))


def test_every_case_links_as_the_table_says(plan_lines):
    got = {}
    for line in plan_lines:
        if line.startswith("case "):
            _, name, *fields = line.split()
            got[name] = dict(f.split("=", 1) for f in fields)
    assert list(got) == [c[0] for c in tc.CASES]
    for name, changes, path, caps, fused, batched, sizes in tc.CASES:
        g = got[name]
        if path.startswith("error:"):
            assert g == {"error": path[len("error:"):]}, name
            continue
        assert g["path"] == path, name
        assert g["caps"].split(",") == caps.split(), name
        # what fused() / batched() answer follows from the path alone
        assert (g["path"] == "frame", g["path"] in ("batch", "batch3")) == (fused, batched), name
        for key, value in sizes.items():
            assert int(g[key]) == value, (name, key)


def test_the_state_block_is_carved_soundly_over_a_grid_of_shapes(plan_lines):
    walked = [line for line in plan_lines if line.startswith("walk ")]
    assert len(walked) == 1 and walked[0].startswith("walk ok ") and int(walked[0].split()[2]) > 5000, walked
