"""Round trips on the steady path of k_batch, read from the built library's gfx950 listing (no GPU needed).

A frame of the batch link is a wave waiting on its own serial chain: what a track wave
issues in a steady frame is ~700 instructions, what it takes is ~8 k cycles.  scripts/k_batch_census.py walks the steady
frame and reports, for every `s_waitcnt lgkmcnt` on it, the scalar loads and LDS accesses the wave can be waiting for there
(`round_trips`).  This pins what round 14 took off the chain:

  * no scalar load is waited for within 8 instructions of its issue (the parent had 5: det_all, the horizons twice, rows /
    rows_capacity, the pointer to the gains);
  * no two scalar loads of a pass fetch the same kernel argument (the parent loaded the horizons twice);
  * at most 4 waits on LDS reads that start a round trip of their own between the loop head and the claim's ds_min_rtn_u64
    (the parent had 6: the frame's count, the grid header, the candidate list, the eight centres, the winner's centre, the
    winner's column; the count and the header are now read a frame ahead, the column with the centre);
  * the GUARD of the written-out scalar loads (batch_link.h, "Kernel arguments a phase ahead"): over the WHOLE listing of the
    kernel and along every path, nothing reads or writes a scalar load's destination registers between the load and the
    first wait for lgkmcnt(0) -- in the built library and in every variant build under scripts/ (the stamps build among
    them), which the measuring scripts run on the GPU;
  * the budget: three waves per SIMD (at most 170 VGPRs), no scratch, no vector spills, scalar spills not above the
    parent's 21, lane moves on the steady path not above the parent's 11.
"""
import importlib.util
import os
import re
import subprocess

import pytest

import test_kernel_resources as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ysmr_amd", "csrc", "libysmr_hip.so")

PARENT_NEAR_SMEM = 5       # scalar loads of the parent's steady path waited for within 8 instructions
PARENT_LDS_ROUNDS = 6
PARENT_SGPR_SPILLS = 21
PARENT_LANE_MOVES = 11
NEAR = 8


def _census():
    spec = importlib.util.spec_from_file_location("k_batch_census", os.path.join(ROOT, "scripts", "k_batch_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(LIB):
        pytest.skip("libysmr_hip.so is not built")
    text = mod.listing_of_library(LIB)
    if text is None:
        pytest.skip("no gfx950 listing of k_batch: llvm-objcopy / llvm-objdump not found")
    c = mod.census(text)
    assert c["kernel instructions"] > 1000 and c["frame"]["instructions"] > 400, "the listing of k_batch looks truncated"
    return mod, c


def _sgprs(operand):
    m = re.fullmatch(r"s(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def test_no_scalar_load_is_waited_for_where_it_is_issued():
    mod, c = _census()
    print(mod.report_round_trips(c))
    loads = mod.smem_waits(c)
    on_path = [k for k, (op, _) in enumerate(c["path"]) if op.startswith("s_load_")]
    assert len(on_path) >= 4, "the walk found no scalar loads: is this k_batch's steady path?"
    assert sorted(i % len(c["path"]) for _, i, _, _ in loads) == on_path, "a scalar load of the steady path meets no wait"
    near = [f"{text} (issued at {i}, waited for at {w})" for w, i, d, text in loads if d <= NEAR]
    assert not near, f"{len(near)} scalar loads waited for within {NEAR} instructions (the parent had {PARENT_NEAR_SMEM}): {near}"


def test_no_kernel_argument_is_loaded_twice_in_a_pass():
    _, c = _census()
    # a pass has one barrier, so the pass IS the interval between two barriers.  Two groups: loads through the kernel
    # argument pointer, and loads through a pointer that was itself loaded on the path (the gains); bytes [start, end)
    pointers, groups = set(), {False: [], True: []}
    for op, args in c["path"]:
        operands = [a.strip() for a in args.split(",")]
        if op.startswith("s_load_dword"):
            dst, base, off = operands[:3]
            width = int(op[len("s_load_dword"):].lstrip("x") or 1)
            start = int(off, 0)
            groups[bool(_sgprs(base)) and _sgprs(base) <= pointers].append((start, start + 4 * width, f"{op} {args}"))
            pointers -= _sgprs(dst)
            if width == 2:
                pointers |= _sgprs(dst)
        elif operands:
            pointers -= _sgprs(operands[0])       # (overwritten by something else)
    twice = [(a[2], b[2]) for g in groups.values() for k, a in enumerate(g) for b in g[k + 1:] if a[0] < b[1] and b[0] < a[1]]
    assert not twice, f"kernel arguments fetched twice in one pass: {twice}"


def test_at_most_four_lds_round_trips_in_front_of_the_claim():
    mod, c = _census()
    rounds = mod.lds_rounds_before_claim(c)
    assert c["path"][c["marks"]["claim"]][0] == "ds_min_rtn_u64"
    assert 1 <= len(rounds) <= 4, f"{len(rounds)} LDS round trips between the loop head and the claim, at {rounds} " \
                                  f"(the parent had {PARENT_LDS_ROUNDS})"


def _libraries():
    import glob
    return [LIB] + sorted(glob.glob(os.path.join(ROOT, "scripts", "var_*.so")))


def test_nothing_touches_a_scalar_loads_registers_before_its_wait():
    spec = importlib.util.spec_from_file_location("k_batch_census", os.path.join(ROOT, "scripts", "k_batch_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(LIB):
        pytest.skip("libysmr_hip.so is not built")
    for lib in _libraries():
        text = mod.listing_of_library(lib)
        if text is None:
            if lib == LIB:
                pytest.skip("no gfx950 listing of k_batch: llvm-objcopy / llvm-objdump not found")
            continue                      # (a variant build of other kernels)
        ins = mod.parse(text)
        loads = [k for k, (op, _, _) in enumerate(ins) if op.startswith("s_load_")]
        assert len(ins) > 1000 and len(loads) >= 8, f"{lib}: the listing of k_batch looks truncated"
        bad = mod.pending_load_hazards(text)
        assert not bad, f"{os.path.relpath(lib, ROOT)}: registers of a scalar load in flight are touched: " + \
                        "; ".join(f"{load} (instruction {i}) <- {what} (instruction {j})" for i, load, j, what in bad)


def _metadata(tmp_path):
    objcopy = R._tool("llvm-objcopy")
    if not os.path.exists(R.LIB):
        pytest.skip("libysmr_hip.so is not built")
    if not objcopy or not R._tool("llvm-readelf"):
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", R.LIB, str(tmp_path / "host.so")], check=True, capture_output=True)
    for k, co in enumerate(R._gfx950_code_objects(fat.read_bytes())):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        notes = subprocess.run([R._tool("llvm-readelf"), "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            if re.search(r"^\s*\.?name:\s+_ZN12_GLOBAL__N_17k_batchENS_10BlKernArgsE\s*$", block, re.M):
                return lambda name: int(re.search(r"\.?" + re.escape(name) + r":\s+(\d+)", block).group(1))
    pytest.fail(f"k_batch not found in the gfx950 code objects of {R.LIB}")


def test_budget_three_waves_per_simd_no_scratch_spills_and_lane_moves_as_the_parent(tmp_path):
    field = _metadata(tmp_path)
    _, c = _census()
    print({n: field(n) for n in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")},
          "lane moves on the steady path:", c["frame"]["lane"])
    assert field("vgpr_count") <= 170, "768 threads need three waves per SIMD"
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
    assert c["frame"]["lane"] <= PARENT_LANE_MOVES, f"{c['frame']['lane']} lane moves on the steady path (the parent had {PARENT_LANE_MOVES})"
    assert field("sgpr_spill_count") <= PARENT_SGPR_SPILLS, f"{field('sgpr_spill_count')} scalar spills (the parent had {PARENT_SGPR_SPILLS})"
