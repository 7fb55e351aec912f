"""Resources of the kernels ``ysmr_mjpeg_encode_batch`` added to csrc/mjpeg.hip or changed in it, read from the built
library's gfx950 code objects (no GPU needed), as test_kernel_mjpeg_resources.py does: no scratch memory, no spilled
register, and the LDS that DESIGN.md ("The annotated video as Motion-JPEG") writes down.  Metadata only; no instruction is
read."""
import re

import test_kernel_mjpeg_resources as base

#: bytes of LDS, as in DESIGN.md: a frame's codes or histogram are 768 words; k_mj_tables holds png_codes.h's Work (7048),
#: 257 counts, 257 lengths, two arrays of 17 words and a count -- 8473 bytes, 8520 as the compiler aligns them
LDS = {"k_mj_blocks": 0, "k_mj_blocks_sampled": 0, "k_mj_hist": 3072, "k_mj_tables": 8520, "k_mj_lengths": 3072, "k_mj_pack": 3072,
       "k_mj_count": 0, "k_mj_layout": 0, "k_mj_write": 0}


def test_the_encoders_kernels_need_no_scratch_and_the_lds_of_the_design(tmp_path, monkeypatch):
    monkeypatch.setattr(base, "KERNELS", tuple(LDS))
    found = base._blocks(tmp_path)
    assert sorted(found) == sorted(LDS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(LDS) - set(found)))
    for kernel, block in found.items():
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        print(kernel, "LDS", lds, "VGPRs", re.search(r"\.?vgpr_count:\s+(\d+)", block).group(1),
              "SGPRs", re.search(r"\.?sgpr_count:\s+(\d+)", block).group(1))
        assert lds == LDS[kernel], f"{kernel}: {lds} bytes of LDS, DESIGN.md says {LDS[kernel]}"
