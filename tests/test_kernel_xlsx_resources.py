"""Resources of the collated workbook's kernels (csrc/xlsx.hip, and ``k_csv_kinds`` of csrc/csv.hip), read from the built
library's gfx950 code objects (no GPU needed), as test_kernel_table_csv_resources.py does for the csv writer, which also holds
the packing kernel the two printers share: both are there, none needs scratch memory or spills a register -- a row's digits are
kept in LDS, integers, cell references and tags are printed straight into their place, a line's kinds stay in registers.  The
row printer's staging is dynamic LDS of at most
what ``ysmr_xlsx_sheet_geometry`` reports; its static LDS (row offsets, a lane's digits) is a few KiB, and both together stay
inside the 64 KiB a workgroup may have.  ``k_csv_kinds`` holds the parse's staged span and nothing else."""
import ctypes
import re

import test_kernel_png_resources as base

KERNELS = ("k_xlsx_rows", "k_csv_kinds")


def test_xlsx_kernels_need_no_scratch_and_only_the_staging_lds(tmp_path, monkeypatch):
    from ysmr_amd import _lib
    rows, staged, longest, span = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ysmr_xlsx_sheet_geometry(ctypes.byref(rows), ctypes.byref(staged), ctypes.byref(longest))
    _lib.lib().ysmr_csv_geometry(None, None, ctypes.byref(span))
    assert rows.value > 0 and rows.value % 64 == 0
    # <row r="1048576">, the index cell, sixteen cells of 27 bytes around a 24-byte value, </row>
    assert longest.value == 17 + 40 + 16 * (27 + 24) + 6
    assert staged.value == rows.value * ((longest.value + 3) // 4 * 4), "the staging holds a workgroup's rows of sixteen widest cells"
    static_limit = {"k_xlsx_rows": 4096, "k_xlsx_pack": 0, "k_csv_kinds": span.value}
    monkeypatch.setattr(base, "KERNELS", KERNELS)
    found = base._blocks(tmp_path)
    assert sorted(found) == sorted(KERNELS), "kernels missing from the gfx950 code objects: {}".format(sorted(set(KERNELS) - set(found)))
    for kernel, block in ((kernel, block) for kernel, blocks in found.items() for block in blocks):
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.?" + field + r":\s+(\d+)", block)
            assert m, f"{field} missing from the metadata of {kernel}"
            print(kernel, field, m.group(1))
            assert int(m.group(1)) == 0, f"{kernel}: {field} = {m.group(1)}"
        lds = int(re.search(r"\.?group_segment_fixed_size:\s+(\d+)", block).group(1))
        print(kernel, "LDS", lds, "VGPRs", re.search(r"\.?vgpr_count:\s+(\d+)", block).group(1), "SGPRs",
              re.search(r"\.?sgpr_count:\s+(\d+)", block).group(1))
        assert lds <= static_limit[kernel], f"{kernel}: {lds} bytes of static LDS"
        assert lds + (staged.value if kernel == "k_xlsx_rows" else 0) <= 65536
