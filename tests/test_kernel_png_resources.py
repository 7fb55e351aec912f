"""Resources of the PNG kernels (csrc/png.hip), read from the built library's gfx950 code objects (no GPU needed): none of
them may need scratch memory -- the parse walks its piece with a lane each, and a map word or a bit buffer kept in a stack
array would go unnoticed otherwise."""
import re
import subprocess

import pytest

from test_kernel_resources import LIB, _gfx950_code_objects, _tool

KERNELS = ("k_png_maps", "k_png_count", "k_png_finish", "k_png_emit", "k_png_stamp")
NAMESPACE = "_ZN12_GLOBAL__N_1"          # png.hip's anonymous namespace: _ZN12_GLOBAL__N_1<len><name>E...


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


def test_png_kernels_need_no_scratch(tmp_path):
    found = _blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, block in ((kernel, block) for kernel, blocks in found.items() for block in blocks):
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert lds <= 32768, f"{kernel}: {lds} bytes of LDS"
