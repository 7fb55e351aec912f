"""CPU-side checks of the C-ABI library: it loads without a GPU and exports every symbol that
include/ysmr_hip.h declares; host-only entry points behave (no compute calls here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from ysmr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_header_symbols_are_exported(lib):
    from ysmr_amd import _lib
    header = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    declared = set(re.findall(r"\b(ysmr_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ysmr_abi_version() == int(re.search(r"#define YSMR_ABI_VERSION\s+(\d+)", header).group(1)) == 15


def test_row_struct_layout():
    from ysmr_amd import _lib
    assert _lib.ROW_DTYPE.itemsize == 40
    assert [_lib.ROW_DTYPE.fields[k][1] for k in ("frame", "track_id", "x", "y", "w", "h", "angle", "disappeared")] == \
        [0, 4, 8, 16, 24, 28, 32, 36]


def test_workspace_size_and_bad_arguments(lib):
    assert lib.ysmr_detect_workspace_bytes(0, 10, 10, 10) == 0
    assert lib.ysmr_detect_workspace_bytes(4, 922, 1228, 2048) > 0
    rc = lib.ysmr_threshold_batch(None, None, 1, 10, 10, 2, 0, 5, 7, 1, None, 0)
    assert rc == 1 and b"channels" in lib.ysmr_last_error()


TABLE_WORKSPACES = {
    # the stages that post-process the finished table carve their workspaces by one rule (csrc/table.h: Arena); the sizes are
    # part of what callers see (they allocate them), and the buffers' order decides where each entry point finds its own
    "ysmr_select_workspace_bytes": {(0, 0): 270848, (1, 0): 270848, (1, 950): 15639040, (2049, 950): 16005888,
                                    (100000, 20000): 152133376, (-1, 0): 0, (2 ** 31, 0): 0},
    "ysmr_evaluate_workspace_bytes": {(0,): 3584, (1,): 3584, (2048,): 139520, (2049,): 143104, (100000,): 6801664, (-1,): 0,
                                      (2 ** 31,): 0},
    "ysmr_plot_workspace_bytes": {(0, 0, 0, 0): 2304, (0, 0, 64, 48): 14336, (1, 1, 64, 48): 14336, (2049, 300, 640, 480): 1252096,
                                  (100000, 3000, 1600, 1200): 8532224, (5, 0, 0, 0): 2304, (1, 1, 32769, 1): 0},
    "ysmr_violin_workspace_bytes": {(0, 1, 0): 4864, (0, 4, 300): 9472, (1, 1, 0): 5888, (1025, 4, 0): 56064,
                                    (100000, 255, 0): 4912384, (0, 64, 32768): 8395008, (0, 0, 0): 0, (0, 256, 0): 0},
}


@pytest.mark.parametrize("name", sorted(TABLE_WORKSPACES))
def test_table_stage_workspace_sizes(lib, name):
    for args, expect in TABLE_WORKSPACES[name].items():
        assert getattr(lib, name)(*args) == expect, (name, args)


def test_gsff_gains_closed_form_matches_reference_formula(lib):
    from oracle.ysmr_oracle import horizon_sizes, lsf_gain
    for fps, n_min, n_max, n_f in [(30.0, 0, 30.0, 3), (29.97, 0, -1.0, 3), (25.0, 4, 24.0, 4)]:
        n_i = (ctypes.c_int32 * n_f)()
        assert lib.ysmr_gsff_gains(fps, n_min, n_max, n_f, n_i, None) == 0
        expect = horizon_sizes(n_min, fps if n_max < 0 else n_max, n_f)
        assert list(n_i) == expect
        total = sum(4 * n for n in expect)
        gains = np.zeros(total)
        assert lib.ysmr_gsff_gains(fps, n_min, n_max, n_f, n_i, gains.ctypes.data) == 0
        off = 0
        for n in expect:
            np.testing.assert_allclose(gains[off:off + 4 * n].reshape(2, 2 * n), lsf_gain(n, 1 / fps)[:2], atol=1e-12)
            off += 4 * n
    n_i = (ctypes.c_int32 * 3)()
    assert lib.ysmr_gsff_gains(30.0, 0, 2.0, 3, n_i, None) == 1      # horizons [0,1,2]: rejected


def test_threshold_params_match_oracle(oracle):
    from ysmr_amd.detect import threshold_params
    for args in [(True, 5, 2.0), (True, 5, 2.5), (True, 3, 0.0), (False, 5, 2.0), (False, 7, 0.5), (True, 0, 1.0)]:
        p = threshold_params(*args)
        assert (p.inv, p.t_low, p.t_high, p.use_high) == oracle.threshold_params(*args)


def _set_order_program(tmp_path, cases):
    """The serial set model of the device code (csrc/set_order.h, what cpython_unused_order runs), compiled for the host as
    tests/set_order_check.cc and run on `cases` = [(m, used columns, table_cap)]: per case the model's return value and order."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "set_order_check")
    built = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ysmr_amd", "csrc"),
                            os.path.join(ROOT, "tests", "set_order_check.cc"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    text = "".join(f"{m} {cap} {len(used)} {' '.join(map(str, sorted(used)))}\n" for m, used, cap in cases)
    done = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and not done.stderr.strip(), done.stderr
    rows = [[int(v) for v in line.split()] for line in done.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [(r[0], r[1:]) for r in rows]


def test_cpython_set_model_matches_this_interpreter(tmp_path):
    rng = np.random.default_rng(0)
    cases = []
    for _ in range(3000):
        m = int(rng.integers(1, 700))
        k = int(rng.integers(0, m + 1))
        cases.append((m, set(int(v) for v in rng.choice(m, size=k, replace=False)), 4096))
    # the unclaimed columns of tests/test_gpu_link.py::test_set_order_when_the_unclaimed_columns_collide, and whole residue
    # classes of the small tables: multiples of 8, 64 and 512
    total = 900
    patterns = [np.arange(0, total, 128), np.arange(0, total, 32), np.arange(7, total, 8)[:90], np.arange(100, 190),
                np.r_[np.arange(0, total, 64), np.arange(300, 345), np.arange(513, 530)],
                np.r_[np.arange(3, total, 16), np.arange(640, 700)], np.arange(total - 70, total),
                np.arange(0, total, 8), np.arange(0, total, 64), np.arange(0, total, 512)]
    for cols in patterns:
        cases.append((total, set(range(total)) - set(int(c) for c in cols), 4096))
    got = _set_order_program(tmp_path, cases)
    for (m, used, _), (n, order) in zip(cases, got):
        expect = list(set(range(0, m)).difference(used))
        assert n == len(expect) and order == expect, (m, sorted(used))
    # a table beyond its capacity: 200 unclaimed columns of 400 grow the table to 512 entries
    (n, order), (n_fits, _) = _set_order_program(tmp_path, [(400, set(range(200, 400)), 256), (400, set(range(200, 400)), 512)])
    assert (n, order) == (-1, []) and n_fits == 200
