"""Resources of the 3-D batch link kernel, read from the built library's gfx950 code object (no GPU needed).

k_batch3 is k_batch without the filter bank, with a third coordinate: like k_batch it has to run three waves per SIMD
(at most 168 VGPRs), use no scratch and spill nothing, and reach its LDS by offset -- a pointer that went through a
structure comes back generic and the compiler then reads LDS with flat loads (batch_link.h, above ``bl_lds``)."""
import re
import subprocess

import pytest

import test_kernel_resources as R

KERNEL = "_ZN12_GLOBAL__N_18k_batch3ENS_11BlKernArgs3E"


def _code_objects(tmp_path):
    objcopy = R._tool("llvm-objcopy")
    if not R.os.path.exists(R.LIB):
        pytest.skip("libysmr_hip.so is not built")
    if not objcopy or not R._tool("llvm-readelf") or not R._tool("llvm-objdump"):
        pytest.skip("llvm-objcopy / llvm-readelf / llvm-objdump not found")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", R.LIB, str(tmp_path / "host.so")], check=True, capture_output=True)
    paths = []
    for k, co in enumerate(R._gfx950_code_objects(fat.read_bytes())):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        paths.append(path)
    return paths


def _notes_and_object(tmp_path):
    for path in _code_objects(tmp_path):
        notes = subprocess.run([R._tool("llvm-readelf"), "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            if re.search(r"^\s*\.?name:\s+" + re.escape(KERNEL) + r"\s*$", block, re.M):
                return block, path
    pytest.fail(f"{KERNEL} (k_batch3) not found in the gfx950 code objects of {R.LIB}")


def _field(block, name):
    m = re.search(r"\.?" + re.escape(name) + r":\s+(\d+)", block)
    assert m, f"{name} missing from the metadata of {KERNEL}"
    return int(m.group(1))


def test_k_batch3_exists_without_scratch_or_spills_and_fits_three_waves_per_simd(tmp_path):
    block, _ = _notes_and_object(tmp_path)
    assert _field(block, "private_segment_fixed_size") == 0
    assert _field(block, "vgpr_spill_count") == 0
    assert _field(block, "sgpr_spill_count") == 0
    assert _field(block, "vgpr_count") <= 168


def test_k_batch3_reaches_lds_and_memory_without_flat_accesses(tmp_path):
    _, path = _notes_and_object(tmp_path)
    dis = subprocess.run([R._tool("llvm-objdump"), "-d", f"--disassemble-symbols={KERNEL}", str(path)], check=True,
                         capture_output=True, text=True).stdout
    body = [ln for ln in dis.splitlines() if re.match(r"^\s+[a-z_0-9]+ ", ln)]
    assert len(body) > 500, "the listing of k_batch3 is empty"
    flat = [ln.strip() for ln in body if re.match(r"^\s+flat_(load|store)", ln)]
    assert not flat, f"{len(flat)} flat accesses in k_batch3, first: {flat[:3]}"
