"""Resources of the TIFF strip kernels (csrc/tiff_decode.hip), read from the built library's gfx950 code objects (no GPU needed):
none of them may need scratch memory -- the LZW table belongs in LDS, 16 KB of positions per strip, and a stack array or a spilled
register in the per-code loop would go unnoticed otherwise -- and none more than 64 KB of LDS.  Metadata only; no instruction is
read."""
import re

import test_kernel_mjpeg_resources as base

KERNELS = ("k_tiff_lzw", "k_tiff_packbits", "k_tiff_copy", "k_tiff_finish")


def test_tiff_kernels_need_no_scratch(tmp_path, monkeypatch):
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
    # the table of k_tiff_lzw IS in LDS: 4096 positions of four bytes and the window of the body
    assert int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", found["k_tiff_lzw"]).group(1)) >= 4096 * 4
