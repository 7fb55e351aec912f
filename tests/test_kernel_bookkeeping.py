"""The bookkeeping of k_batch's steady frame -- claims, ranks + row, ageing -- read from the built library's gfx950 listing
(no GPU needed).

Between the search and the filter bank a track wave settles its claim, requests what the filter bank will need, writes
the row of the frame before and ages.  Every instruction there is paid in the chain of the wave that paces the frame and
three times in the issue slots of its SIMD.  scripts/k_batch_census.py walks the steady
frame; this pins its three lines where round 15 left them, and the frame's budget:

  * claims <= 62, ranks + row <= 61, ageing <= 65 (the parent: 90 / 71 / 77, profiles/r15_census_base.log);
  * two exec regions between the claim's atomic and barrier A: the tie flag and ONE region for the three filters' leaving
    measurements (the parent: six -- the flag, the box, `alive`, and one per filter);
  * at most 168 VGPRs, no scratch, no vector spills, scalar spills <= 20, lane moves on the steady path <= 10 (the
    parent's figures), one s_barrier on the walked path, no scalar load waited for within 8 instructions, at most three
    LDS round trips in front of the claim, no register of a scalar load in flight touched, and a filter bank no larger
    than the parent's 190 instructions.
"""
import importlib.util
import os

import pytest

import test_kernel_round_trips as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ysmr_amd", "csrc", "libysmr_hip.so")

PARENT = {"claims": 90, "ranks + row": 71, "ageing": 77}
REACHED = {"claims": 62, "ranks + row": 61, "ageing": 65}
PARENT_FILTER_BANK = 190
PARENT_REGIONS, REACHED_REGIONS = 6, 2
PARENT_SGPR_SPILLS, PARENT_LANE_MOVES = 20, 10


def _listing():
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
    return mod, text, c


def test_claims_row_and_ageing_stay_where_round_15_left_them():
    mod, _, c = _listing()
    print(mod.report(c))
    assert c["claims"]["ops"][0] == "ds_min_rtn_u64", "the walk did not find the claim"
    assert sum(o == "global_store_dwordx4" for o in c["ranks + row"]["ops"]) >= 2, "the walk did not find the row"
    for name, reached in REACHED.items():
        assert reached <= PARENT[name]
        assert c[name]["instructions"] <= reached, \
            f"{name}: {c[name]['instructions']} instructions on the steady path, round 15 reached {reached} (its parent had {PARENT[name]})"
    assert sum(REACHED.values()) < sum(PARENT.values())
    assert c["filter bank"]["instructions"] <= PARENT_FILTER_BANK


def test_one_exec_region_for_the_leaving_measurements():
    _, _, c = _listing()
    a, b = c["marks"]["claim"], c["marks"]["barrier A"]
    regions = [(k, op) for k, (op, _) in enumerate(c["path"][a:b], a) if "saveexec" in op]
    loads = [op for op, _ in c["path"][a:b] if op.startswith("global_load") and not op.startswith("global_load_lds")]
    assert len(loads) >= 4, "the leaving measurements and the box are not requested in front of barrier A"
    assert len(regions) <= REACHED_REGIONS, f"{len(regions)} exec regions between the claim's atomic and barrier A: {regions} " \
                                            f"(round 15 reached {REACHED_REGIONS}, its parent had {PARENT_REGIONS})"
    # nothing zeroes a leaving measurement or the box on the steady path: the line of zeros is read, not written
    zeroed = [args for op, args in c["path"][a:b] if op == "v_mov_b64_e32" and args.replace(" ", "").endswith(",0")]
    assert len(zeroed) <= 1, f"64-bit zeros written between the claim and barrier A: {zeroed}"


def test_budget_of_the_frame(tmp_path):
    mod, text, c = _listing()
    field = T._metadata(tmp_path)
    figures = {n: field(n) for n in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
    print(figures, "lane moves:", c["frame"]["lane"])
    assert figures["vgpr_count"] <= 168, "768 threads need three waves per SIMD"
    assert figures["private_segment_fixed_size"] == 0 and figures["vgpr_spill_count"] == 0
    assert figures["sgpr_spill_count"] <= PARENT_SGPR_SPILLS
    assert c["frame"]["lane"] <= PARENT_LANE_MOVES
    assert c["barriers"] == 1, f"{c['barriers']} s_barrier on the walked path"
    near = [t for t in mod.smem_waits(c) if t[2] <= 8]
    assert not near, f"scalar loads waited for within 8 instructions: {near}"
    rounds = mod.lds_rounds_before_claim(c)
    assert 1 <= len(rounds) <= 3, f"{len(rounds)} LDS round trips in front of the claim, at {rounds}"
    assert mod.pending_load_hazards(text) == []
