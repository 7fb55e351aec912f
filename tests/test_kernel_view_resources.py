"""Resources of the detection view's kernels (csrc/view.hip), read from the built library's gfx950 code objects (no GPU
needed): neither may need scratch memory -- a spilled register or a stack array in a per-pixel loop would go unnoticed
otherwise -- nor LDS, and their registers must fit their launch bounds with room to spare: 256 threads are one wave per SIMD,
and at 128 vector registers or fewer four such workgroups share a compute unit."""
import re
import subprocess

import pytest

from test_kernel_resources import LIB, _gfx950_code_objects, _tool

KERNELS = ("k_view_boxes", "k_view_tracks")
NAMESPACE = "_ZN12_GLOBAL__N_1"          # view.hip's anonymous namespace


def _blocks(tmp_path):
    import os
    objcopy, readelf = _tool("llvm-objcopy"), _tool("llvm-readelf")
    if not os.path.exists(LIB):
        pytest.skip("libysmr_hip.so is not built")
    if not objcopy or not readelf:
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "host.so")], check=True, capture_output=True)
    found = {}
    for k, co in enumerate(_gfx950_code_objects(fat.read_bytes())):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            m = re.search(r"^\s*\.?name:\s+(\S+)\s*$", block, re.M)
            if not m:
                continue
            for kernel in KERNELS:
                if m.group(1).startswith(NAMESPACE + str(len(kernel)) + kernel + "E"):
                    found.setdefault(kernel, []).append(block)
    return found


def _field(block, field, kernel):
    m = re.search(r"\.?" + field + r":\s+(\d+)", block)
    assert m, f"{field} missing from the metadata of {kernel}"
    return int(m.group(1))


def test_view_kernels_need_no_scratch_and_fit_their_launch_bounds(tmp_path):
    found = _blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, blocks in found.items():
        assert len(blocks) == 1, kernel
        block = blocks[0]
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size"):
            assert _field(block, field, kernel) == 0, f"{kernel}: {field} = {_field(block, field, kernel)}"
        # (k_view_boxes evaluates cos and sin in float64, as k_luminosity does for the same corners: the argument reduction's
        # constants take more scalar registers than there are, and the compiler parks some in the lanes of a vector register --
        # no memory is involved, private_segment_fixed_size above says so.  The track painter has no such excuse.)
        if kernel == "k_view_tracks":
            assert _field(block, "sgpr_spill_count", kernel) == 0, kernel
        assert _field(block, "max_flat_workgroup_size", kernel) == 256, kernel
        assert _field(block, "wavefront_size", kernel) == 64, kernel
        assert _field(block, "vgpr_count", kernel) <= 128, f"{kernel}: {_field(block, 'vgpr_count', kernel)} VGPRs"
        assert _field(block, "sgpr_count", kernel) <= 106, f"{kernel}: {_field(block, 'sgpr_count', kernel)} SGPRs"
