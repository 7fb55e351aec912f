"""Resources of the kernels of ysmr_png_deflate_dynamic (csrc/png.hip), read from the built library's gfx950 code objects (no
GPU needed), as test_kernel_png_resources.py does for the fixed stream's: no scratch memory, no spills -- the code
construction keeps every array in LDS -- and at most 32 KiB of LDS."""
import re

import test_kernel_png_resources as base

KERNELS = ("k_png_dmaps", "k_png_dhist", "k_png_dcodes", "k_png_dsize", "k_png_dfinish", "k_png_demit")


def test_dynamic_png_kernels_need_no_scratch(tmp_path, monkeypatch):
    monkeypatch.setattr(base, "KERNELS", KERNELS)
    found = base._blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, block in ((kernel, block) for kernel, blocks in found.items() for block in blocks):
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert lds <= 32768, f"{kernel}: {lds} bytes of LDS"
        print(kernel, "LDS", lds, "VGPRs", re.search(r"\.?vgpr_count:\s+(\d+)", block).group(1))
