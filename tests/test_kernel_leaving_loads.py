"""The measurements that leave the filters' windows come with ONE 16-byte load each (batch_link.h: bl_ring_issue16), read
from the built library's gfx950 listing (no GPU needed).

A track wave requested them with six 8-byte loads; as three 16-byte loads outside the compiler's books a steady pass
holds 8 vector-memory instructions instead of 11 (the claimed box, the three entries, the row's three stores of the frame
before, the ring store), and the kernel as a whole three loads fewer.  The bound on the kernel's loads leaves room for two
more than it has today: a warm-up by the waves without a track was allowed two static loads of its own."""
import importlib.util
import os
import sys

import pytest

from test_kernel_listing import _k_batch_listing, _mnemonics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_VECTOR_LOADS = 45
STEADY_VECTOR_MEMORY = 8


def _census_module():
    spec = importlib.util.spec_from_file_location("k_batch_census", os.path.join(ROOT, "scripts", "k_batch_census.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules.setdefault("k_batch_census", mod)
    spec.loader.exec_module(mod)
    return mod


def test_k_batch_has_at_most_45_vector_memory_loads(tmp_path):
    ops = _mnemonics(_k_batch_listing(tmp_path))
    loads = [o for o in ops if o.startswith(("global_load", "buffer_load", "flat_load")) and not o.startswith("global_load_lds")]
    print(f"k_batch: {len(loads)} vector-memory loads")
    assert len(ops) > 1000, "the listing of k_batch looks truncated"
    assert len(loads) <= MAX_VECTOR_LOADS, f"{len(loads)} vector-memory loads in k_batch"


def test_the_steady_pass_holds_eight_vector_memory_instructions(tmp_path):
    mod = _census_module()
    listing = _k_batch_listing(tmp_path)
    c = mod.census("0000000000000000 <" + mod.KERNEL + ">:\n" + listing)
    vmem = [" ".join(line) for line in c["path"] if "vmem" in mod.classify(line[0])]
    print("\n".join(vmem))
    assert c["frame"]["vmem"] == len(vmem) == STEADY_VECTOR_MEMORY, vmem
    wide = [v for v in vmem if v.startswith("global_load_dwordx4") and " sc1" in v]
    assert len(wide) == 3, f"the three leaving entries as 16-byte loads past L1: {wide}"
    assert not [v for v in vmem if v.startswith("global_load_dwordx2")], "an 8-byte ring load is back on the steady pass"


def test_nothing_touches_a_written_out_ring_load_before_the_wait(tmp_path):
    """The guard of bl_ring_issue16: along every path from each written-out 16-byte load to its vmcnt(0) wait nothing reads,
    copies or overwrites the registers it lands in (scripts/k_batch_census.py: pending_load_hazards, which covers the
    written-out scalar loads as well)."""
    mod = _census_module()
    listing = "0000000000000000 <" + mod.KERNEL + ">:\n" + _k_batch_listing(tmp_path)
    followed = [a for o, a, _ in mod.parse(listing) if o == "global_load_dwordx4" and " sc1" in a]
    assert len(followed) >= 3, followed
    assert mod.pending_load_hazards(listing) == []
