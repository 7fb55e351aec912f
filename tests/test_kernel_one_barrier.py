"""One workgroup barrier per steady frame of k_batch, read from the built library's gfx950 listing (no GPU needed).

scripts/k_batch_census.py walks a pass of the frame loop the way a steady frame runs it (guarded rare blocks skipped:
the exact claim path and the registration, with barriers of their own, are such blocks).  The walked path must hold
exactly ONE s_barrier, barrier A behind the claim's atomic; the frame's other barrier, at its end, is gone
(DESIGN.md section 4, round 12).

Not pinned: "no s_waitcnt vmcnt(0) in a track wave's path".  A track wave has one, in front of the filter bank, for the
measurements that leave its windows and the claimed box -- loads requested in front of barrier A, a barrier and the
ageing old; it is in the listing for every wave, and whether the wait in front of barrier A (which only the waves that
requested a grid block take) is skipped by a track wave is decided at run time, not in the listing.  What the listing
does say, and this checks: the wait in front of the barrier sits in a guarded block of its own (the walk skips it), and
between barrier A and the filter bank's reciprocal the walked path waits for vector memory once.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ysmr_amd", "csrc", "libysmr_hip.so")


def _census():
    spec = importlib.util.spec_from_file_location("k_batch_census", os.path.join(ROOT, "scripts", "k_batch_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(LIB):
        pytest.skip("libysmr_hip.so is not built")
    text = mod.listing_of_library(LIB)
    if text is None:
        pytest.skip("no gfx950 listing of k_batch: llvm-objcopy / llvm-objdump not found")
    return mod, mod.census(text)


def test_steady_frame_has_one_barrier():
    mod, c = _census()
    print(mod.report(c))
    assert c["frame"]["instructions"] > 400, "the listing of k_batch looks truncated"
    assert c["barriers"] == 1
    ops = [op for op, _ in c["path"]]
    claim, bar = c["marks"]["claim"], c["marks"]["barrier A"]
    assert ops[bar] == "s_barrier" and claim < bar, "the one barrier is barrier A, behind the claim's atomic"
    assert "s_barrier" not in ops[:claim] and "s_barrier" not in ops[bar + 1:]


def test_track_wave_waits_for_vector_memory_once_per_frame():
    mod, c = _census()
    path, marks = c["path"], c["marks"]
    waits = [k for k, (op, args) in enumerate(path) if op == "s_waitcnt" and "vmcnt(0)" in args]
    assert len(waits) == 1, f"s_waitcnt vmcnt(0) on the walked path at {waits}"
    assert marks["row end"] <= waits[0] < marks["filter bank end"], "the wait is the one in front of the filter bank"
    assert "vmcnt" not in " ".join(args for op, args in path[marks["claim"]:marks["barrier A"] + 1] if op == "s_waitcnt"), \
        "a track wave beside helper waves waits for no vector memory access in front of barrier A"
