"""The steady path of k_batch's filter bank, read from the built library's gfx950 listing (no GPU needed).

A frame of the batch link lasts as long as one SIMD needs to issue the vector instructions of the three track waves it
carries, so an instruction that runs in every frame of every track wave and serves a case that
occurs in three frames of a track's life is paid for in the headline.  scripts/k_batch_census.py walks the kernel's frame
loop the way a steady frame runs it (guarded rare blocks skipped) and counts per phase; this pins the filter bank's line:

  * no v_readlane_b32 of a spilled horizon n_i: the mode cascade sits behind one compare of the history length;
  * the selects on `full` / `fresh`, the clamp's and the cascade's are gone (at most 8 v_cndmask_b32 may come back);
  * the vector instruction count stays where the change left it.

The figures are the census's own ("filter bank" line).  Its "by hand" line adds what a hand count of the parent included
beyond the steady path -- 242 there, 218 on the path itself: profiles/r11_census_base.log.
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ysmr_amd", "csrc", "libysmr_hip.so")

PARENT_VALU = 218          # the parent's steady path (242 by the hand count that included the seeding block's tail)
PARENT_CNDMASK = 37
PARENT_LANE = 12
REACHED_VALU = 158         # this change: 148 float64, 6 v_mov, 1 compare, 1 lane move, 2 others
REACHED_LANE = 1           # the ring store's seat stride, spilled in the prologue


def _sgprs(operand):
    """The scalar registers an operand names: s7 -> {7}, s[4:5] -> {4, 5}."""
    m = re.fullmatch(r"-?s(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"-?s\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


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


def test_filter_bank_steady_path_carries_no_rare_case_code():
    mod, c = _census()
    print(mod.report(c))
    fb = c["filter bank"]
    assert c["kernel instructions"] > 1000 and c["frame"]["instructions"] > 400, "the listing of k_batch looks truncated"
    assert fb["f64"] >= 120 and "v_div_fixup_f64" in fb["ops"], "the walk did not find the filter bank"
    assert REACHED_VALU <= PARENT_VALU - 40
    assert fb["valu"] <= REACHED_VALU, f"{fb['valu']} vector instructions in the filter bank's steady path, the change reached {REACHED_VALU}"
    assert fb["cndmask"] <= 8, f"{fb['cndmask']} v_cndmask_b32 in the filter bank's steady path (the parent had {PARENT_CNDMASK})"
    # the mode cascade compared the history length with n_i out of spilled scalar registers: v_readlane_b32 sX, then a
    # v_cmp of sX with a vector register.  No lane move of the steady path may feed a compare.
    fed, cmp_uses = set(), []
    for op, args in fb["lines"]:
        operands = [a.strip() for a in args.split(",")]
        if op.startswith("v_cmp") and fed & set().union(*map(_sgprs, operands)):
            cmp_uses.append(f"{op} {args}")
        if op.startswith("v_readlane"):
            fed |= _sgprs(operands[0])
        elif operands:
            fed -= _sgprs(operands[0])            # (overwritten by something else)
    assert not cmp_uses, f"a spilled scalar feeds a compare in the filter bank's steady path: {cmp_uses}"
    assert fb["lane"] <= REACHED_LANE, f"{fb['lane']} lane moves in the filter bank's steady path (the parent had {PARENT_LANE})"


def test_census_phases_add_up():
    mod, c = _census()
    total = sum(c[name]["instructions"] for name in mod.PHASES)
    assert total == c["frame"]["instructions"]
    for name in mod.PHASES:
        assert c[name]["instructions"] > 0, f"empty phase {name}"
    assert "ds_min_rtn_u64" in c["claims"]["ops"] or c["claims"]["ops"][0] == "ds_min_rtn_u64"
    assert sum(o == "global_store_dwordx4" for o in c["ranks + row"]["ops"]) >= 2, "the row's stores are not on the walked path"
