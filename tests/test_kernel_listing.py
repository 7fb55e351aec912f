"""Memory instructions of the batch link kernel, read from the built library's gfx950 listing (no GPU needed).

k_batch addresses LDS by offset and global memory by segment (batch_link.h, above bl_lds): a pointer that lost its
address space comes back as flat_load / flat_store, which takes the vector-memory path AND counts on lgkmcnt, so one
of them inside the frame loop puts a full memory round trip into every wave's frame.  The twelve gain constants of the
filter bank were read that way (six flat_load_dwordx4 per wave and frame) until they moved to scalar loads through a
constant-address-space pointer.  This disassembles the kernel and checks that none is back, and that the kernel as a
whole has no more vector-memory loads than it had before that change."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import KERNEL, LIB, _gfx950_code_objects, _tool

# global_load* instructions in k_batch's listing at the commit before the gains left vector memory ("Luminosity as a
# third tracking coordinate"): 48, of which 2 are the LDS-DMA global_load_lds_dwordx4, beside 12 flat_load_dwordx4.
# The DMA is counted apart on both sides.  A change that brings a vector-memory load back into the kernel has to raise
# this figure, and say why.
PARENT_GLOBAL_LOADS = 48
PARENT_LDS_DMA = 2


def _k_batch_listing(tmp_path):
    objcopy, objdump = _tool("llvm-objcopy"), _tool("llvm-objdump")
    if not os.path.exists(LIB):
        pytest.skip("libysmr_hip.so is not built")
    if not objcopy or not objdump:
        pytest.skip("llvm-objcopy / llvm-objdump not found")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "host.so")], check=True,
                   capture_output=True)
    for k, co in enumerate(_gfx950_code_objects(fat.read_bytes())):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        text = subprocess.run([objdump, "-d", f"--disassemble-symbols={KERNEL}", str(path)], check=True,
                              capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <" + re.escape(KERNEL) + r">:\n", text, re.M)
        if m:
            body = text[m.end():]
            end = re.search(r"^[0-9a-f]+ <[^>]+>:\n", body, re.M)      # (the next symbol, should the tool go on)
            return body[:end.start()] if end else body
    pytest.fail(f"{KERNEL} not found in the gfx950 code objects of {LIB}")


def _mnemonics(listing):
    """The mnemonic of every instruction line of an llvm-objdump listing."""
    out = []
    for line in listing.splitlines():
        m = re.match(r"\s+([a-z][a-z0-9_]*)\b", line)
        if m:
            out.append(m.group(1))
    return out


def test_k_batch_has_no_flat_access_and_no_new_vector_loads(tmp_path):
    ops = _mnemonics(_k_batch_listing(tmp_path))
    assert len(ops) > 1000, "the listing of k_batch looks truncated"
    assert any(o.startswith("ds_read") for o in ops) and any(o == "s_barrier" for o in ops)
    flat = [o for o in ops if o.startswith("flat_load") or o.startswith("flat_store")]
    dma = [o for o in ops if o.startswith("global_load_lds")]
    loads = [o for o in ops if o.startswith(("global_load", "buffer_load", "flat_load")) and not o.startswith("global_load_lds")]
    print(f"k_batch: {len(ops)} instructions, {len(loads)} vector-memory loads, {len(dma)} LDS-DMA, {len(flat)} flat")
    assert not flat, f"flat accesses in k_batch: {sorted(set(flat))}"
    limit = PARENT_GLOBAL_LOADS - PARENT_LDS_DMA
    assert len(loads) <= limit, f"{len(loads)} vector-memory loads in k_batch, the parent had {limit}"
    assert len(dma) <= PARENT_LDS_DMA, f"{len(dma)} LDS-DMA instructions in k_batch, the parent had {PARENT_LDS_DMA}"
