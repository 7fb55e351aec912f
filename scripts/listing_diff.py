#!/usr/bin/env python3
"""Did a change leave the kernels alone?  python scripts/listing_diff.py OLD.so NEW.so [-v]

For every kernel of the two libraries' gfx950 code objects: whether the disassembly is the same (llvm-objdump -d with
addresses and encodings stripped, so that code which only moved compares equal) and whether the resource notes are
(VGPRs, SGPRs, scratch, LDS, spills).  Device functions that are not kernels (cpython_unused_order) are listed the same
way, marked "function".  Prints one line per symbol that differs or exists on one side only, then the counts; with -v
a unified diff of every listing that differs.  Exit status 1 when anything differs.  No GPU needed.

The code objects are taken out of the library the way tests/test_kernel_resources.py does it.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_kernel_resources import _gfx950_code_objects, _tool  # noqa: E402

NOTES = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
         "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size")


def symbols_of(lib):
    """{symbol: (listing lines, notes or None)} over the library's gfx950 code objects; notes only for kernels."""
    objcopy, objdump, readelf = _tool("llvm-objcopy"), _tool("llvm-objdump"), _tool("llvm-readelf")
    if not (objcopy and objdump and readelf):
        raise SystemExit("llvm-objcopy / llvm-objdump / llvm-readelf not found")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(tmp, "host.so")], check=True, capture_output=True)
        for k, co in enumerate(_gfx950_code_objects(open(fat, "rb").read())):
            path = os.path.join(tmp, f"co{k}.o")
            with open(path, "wb") as fh:
                fh.write(co)
            notes = {}
            text = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s+- \.", text):
                name = re.search(r"^\s*\.?name:\s+(\S+)\s*$", block, re.M)
                if name and re.search(r"\.?vgpr_count:", block):
                    notes[name.group(1)] = {f: int(m.group(1)) for f in NOTES for m in [re.search(r"\.?" + f + r":\s+(\d+)", block)] if m}
            sym = None
            for line in subprocess.run([objdump, "-d", path], check=True, capture_output=True, text=True).stdout.splitlines():
                head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if head:
                    sym = head.group(1)
                    out[sym] = ([], notes.get(sym))
                elif sym and line.startswith("\t"):
                    out[sym][0].append(re.sub(r"\s*//.*$", "", line).strip())     # "// ADDRESS: ENCODING <symbol+0xOFFSET>" goes
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    if len(args) != 2:
        raise SystemExit(__doc__)
    old, new = symbols_of(args[0]), symbols_of(args[1])
    same = differ = 0
    for sym in sorted(set(old) | set(new)):
        kind = "kernel" if (old.get(sym) or new.get(sym))[1] is not None else "function"
        if sym not in old or sym not in new:
            print(f"{kind} {sym}: only in {'NEW' if sym in new else 'OLD'}")
            differ += 1
            continue
        (lo, no), (ln, nn) = old[sym], new[sym]
        if lo == ln and no == nn:
            same += 1
            continue
        differ += 1
        what = [] if lo == ln else [f"listing differs ({len(lo)} -> {len(ln)} instructions)"]
        if no != nn:
            what.append("notes differ: " + ", ".join(f"{f} {no.get(f)} -> {nn.get(f)}" for f in NOTES if (no or {}).get(f) != (nn or {}).get(f)))
        print(f"{kind} {sym}: " + "; ".join(what))
        if "-v" in sys.argv and lo != ln:
            print("\n".join(difflib.unified_diff(lo, ln, "OLD", "NEW", lineterm="", n=2)))
    print(f"{same} symbols identical (listing and notes), {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
