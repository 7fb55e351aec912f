"""Register budget of the batch link kernel, read from the built library (no GPU needed).

k_batch runs three waves per SIMD (168 VGPRs at most).  A spilled vector register costs a scratch store and load inside
the frame loop, and one can come back unnoticed with any change to the kernel: this reads the gfx950 code object's
metadata out of libysmr_hip.so and checks the figures.  Scalar registers spilled into vector lanes are not checked: the
ones left are used on rarely taken paths, and removing them by reading the kernel arguments again where they are used
made the link slower."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ysmr_amd", "csrc", "libysmr_hip.so")
KERNEL = "_ZN12_GLOBAL__N_17k_batchENS_10BlKernArgsE"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def _gfx950_code_objects(fatbin):
    """The gfx950 code objects of every offload bundle in a .hip_fatbin section (one bundle per translation unit)."""
    out = []
    at = fatbin.find(BUNDLE_MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", fatbin, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, p)
            triple = fatbin[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.endswith("gfx950") and size:
                out.append(fatbin[at + off:at + off + size])
        at = fatbin.find(BUNDLE_MAGIC, at + 1)
    return out


def _kernel_notes(tmp_path):
    objcopy, readelf = _tool("llvm-objcopy"), _tool("llvm-readelf")
    if not os.path.exists(LIB):
        pytest.skip("libysmr_hip.so is not built")
    if not objcopy or not readelf:
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "host.so")], check=True,
                   capture_output=True)
    for k, co in enumerate(_gfx950_code_objects(fat.read_bytes())):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        # the metadata lists each kernel as one YAML mapping; take the one whose .name is k_batch
        for block in re.split(r"\n\s+- \.", notes):
            if re.search(r"^\s*\.?name:\s+" + re.escape(KERNEL) + r"\s*$", block, re.M):
                return block
    pytest.fail(f"{KERNEL} not found in the gfx950 code objects of {LIB}")


def _field(block, name):
    m = re.search(r"\.?" + re.escape(name) + r":\s+(\d+)", block)
    assert m, f"{name} missing from the metadata of {KERNEL}"
    return int(m.group(1))


def test_k_batch_needs_no_scratch_and_fits_three_waves_per_simd(tmp_path):
    block = _kernel_notes(tmp_path)
    assert _field(block, "vgpr_spill_count") == 0
    assert _field(block, "private_segment_fixed_size") == 0
    assert _field(block, "vgpr_count") <= 168
