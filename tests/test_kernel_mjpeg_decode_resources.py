"""Resources of the Motion-JPEG decode kernels (csrc/mjpeg_decode.hip), read from the built library's gfx950 code objects (no
GPU needed): none of them may need scratch memory or spill a register -- the symbol loop of the entropy kernel is serial work
on one lane per restart interval, and a stack array or a spilled register inside it would go unnoticed otherwise.  Metadata
only; no instruction is read."""
import re

import test_kernel_mjpeg_resources as base

KERNELS = ("k_mjd_headers", "k_mjd_markers", "k_mjd_entropy", "k_mjd_idct", "k_mjd_colour")


def test_mjpeg_decode_kernels_need_no_scratch(tmp_path, monkeypatch):
    monkeypatch.setattr(base, "KERNELS", KERNELS)
    found = base._blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, block in found.items():
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert lds <= 65536, f"{kernel}: {lds} bytes of LDS"
