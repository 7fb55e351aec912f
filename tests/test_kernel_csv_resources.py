"""Resources of the device csv reader's kernels (csrc/csv.hip), read from the built library's gfx950 code objects (no GPU
needed), as test_kernel_png_dynamic_resources.py does for the PNG kernels: all five are there, none needs scratch memory or
spills a register -- a line's seven values and the parser's state stay in registers -- and the LDS is what the staging needs:
the staged span of the parse (``ysmr_csv_geometry``) and a few words for the counts of the index passes."""
import ctypes
import re

import test_kernel_png_resources as base

KERNELS = ("k_csv_index", "k_csv_starts", "k_csv_parse", "k_csv_keys", "k_csv_gather")


def test_csv_kernels_need_no_scratch_and_only_the_staging_lds(tmp_path, monkeypatch):
    from ysmr_amd import _lib
    span = ctypes.c_int(0)
    _lib.lib().ysmr_csv_geometry(None, None, ctypes.byref(span))
    lds_limit = {"k_csv_index": 64, "k_csv_starts": 64, "k_csv_parse": span.value, "k_csv_keys": 0, "k_csv_gather": 0}
    assert 0 < span.value <= 65536
    monkeypatch.setattr(base, "KERNELS", KERNELS)
    found = base._blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, block in ((kernel, block) for kernel, blocks in found.items() for block in blocks):
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        print(kernel, "LDS", lds, "VGPRs", re.search(r"\.?vgpr_count:\s+(\d+)", block).group(1), "SGPRs",
              re.search(r"\.?sgpr_count:\s+(\d+)", block).group(1))
        assert lds <= lds_limit[kernel], f"{kernel}: {lds} bytes of LDS, the staging needs {lds_limit[kernel]}"
