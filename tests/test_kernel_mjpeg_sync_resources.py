"""Resources of the kernels ``ysmr_mjpeg_decode_batch_sync`` adds (csrc/mjpeg_decode.hip), read from the built library's gfx950
code objects (no GPU needed): none of them may need scratch memory or spill a register -- k_mjd_sync decodes every subsequence
several times, symbol by symbol, and a stack array or a spilled register inside that loop would go unnoticed otherwise -- and
the frame's tables with a pass's states must fit the LDS.  Metadata only; no instruction is read."""
import re

import test_kernel_mjpeg_resources as base

KERNELS = ("k_mjd_destuff", "k_mjd_sync", "k_mjd_dc")


def test_mjpeg_sync_kernels_need_no_scratch(tmp_path, monkeypatch):
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
