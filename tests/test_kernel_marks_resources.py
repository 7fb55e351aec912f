"""Resources of the typed csv parse (csrc/csv.hip: k_csv_parse_typed) and of the kernels that build the annotated video's
marks (csrc/marks.hip), read from the built library's gfx950 code objects (no GPU needed), as test_kernel_csv_resources.py
does for the seven-column reader: all four are there, none needs scratch memory or spills a register -- a line's up to
sixteen values stay in registers, picked by compares and never by an index -- and the typed parse's LDS is at most the staged
span (``ysmr_csv_geometry``); the marks kernels need none."""
import ctypes
import re

import test_kernel_png_resources as base

KERNELS = ("k_csv_parse_typed", "k_marks_keys", "k_marks_gather", "k_marks_first")


def test_typed_parse_and_marks_kernels_need_no_scratch_and_only_the_staging_lds(tmp_path, monkeypatch):
    from ysmr_amd import _lib
    span = ctypes.c_int(0)
    _lib.lib().ysmr_csv_geometry(None, None, ctypes.byref(span))
    assert 0 < span.value <= 65536
    lds_limit = {"k_csv_parse_typed": span.value, "k_marks_keys": 0, "k_marks_gather": 0, "k_marks_first": 0}
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
        assert lds <= lds_limit[kernel], f"{kernel}: {lds} bytes of LDS, the limit is {lds_limit[kernel]}"
