"""Resources of the table writer's kernels (csrc/table_csv.hip), read from the built library's gfx950 code objects (no GPU
needed), as test_kernel_csv_resources.py does for the reader: all four are there.  The steady kernels -- the pre-pass, the row
printer and the packing launch -- need no scratch memory and spill no register: a row's digits are kept in LDS, integers are
printed straight into their place.  ``k_table_wide`` prints the rare cell with multi-word integers and is exempt from the
scratch condition, and from that one only.  The row printer's staging is dynamic LDS of at most what
``ysmr_table_format_geometry`` reports; its static LDS (row offsets, a lane's digits) is a few KiB, and both together stay
inside the 64 KiB a workgroup may have."""
import ctypes
import re

import test_kernel_png_resources as base

KERNELS = ("k_table_prepass", "k_table_wide", "k_table_rows", "k_table_pack")
MAY_USE_SCRATCH = ("k_table_wide",)


def test_table_kernels_need_no_scratch_and_only_the_staging_lds(tmp_path, monkeypatch):
    from ysmr_amd import _lib
    rows, staged = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_table_format_geometry(ctypes.byref(rows), ctypes.byref(staged))
    assert rows.value > 0 and rows.value % 64 == 0
    assert staged.value == rows.value * 16 * 25, "the staging holds a workgroup's rows of sixteen widest fields"
    static_limit = {"k_table_prepass": 0, "k_table_wide": 0, "k_table_rows": 8192, "k_table_pack": 0}
    monkeypatch.setattr(base, "KERNELS", KERNELS)
    found = base._blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, block in ((kernel, block) for kernel, blocks in found.items() for block in blocks):
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            print(kernel, field, m.group(1))
            if field == "private_segment_fixed_size" and kernel in MAY_USE_SCRATCH:
                continue
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        print(kernel, "LDS", lds, "VGPRs", re.search(r"\.?vgpr_count:\s+(\d+)", block).group(1), "SGPRs",
              re.search(r"\.?sgpr_count:\s+(\d+)", block).group(1))
        assert lds <= staged.value, f"{kernel}: {lds} bytes of LDS, more than the staging"
        assert lds <= static_limit[kernel], f"{kernel}: {lds} bytes of static LDS"
        assert lds + (staged.value if kernel == "k_table_rows" else 0) <= 65536
