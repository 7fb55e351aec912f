#!/usr/bin/env python3
"""Hot-path census of k_batch: what a track wave issues in a steady frame, read off the gfx950 listing (no GPU needed).

    python scripts/k_batch_census.py [ysmr_amd/csrc/libysmr_hip.so | track.s | k_batch.dis]

The argument is the built library (its gfx950 code object is disassembled with llvm-objdump), a listing that llvm-objdump -d
wrote, or the compiler's own -S output.  The walk starts at the head of the frame loop and follows the steady frame:

  * it falls through, and follows unconditional branches;
  * a FORWARD conditional branch (s_cbranch_execz / vccz / vccnz / scc0 / scc1) jumps over a guarded block.  The block is
    skipped -- it is a rare path: the 3 x 3 search, the quadrant list of a split cell, the wave search, the exact claims, the
    registration, the seeding of a new track, a filter bank that grows, the block that gives up a track wave (its landmark:
    three or more s_barrier around a 16-byte load and a 16-byte store, the ring copy) -- unless it holds one of the landmarks below (the blocks under `propose`, `alive` and
    the row's bounds check ARE the steady frame) or vector-memory loads without a barrier or a loop (the ring entries that
    leave the windows, the claimed detection's box);
  * of an if / else (s_andn2_saveexec / s_or_saveexec between the halves) whose first half was skipped, the second half
    is the steady one (the candidate list's search, behind the 3 x 3 block search);
  * a forward s_cbranch_execnz leads to a rare block laid out of line, and a backward branch closes an inner loop (the ring
    stores of a seeding, a run's later candidates): neither is taken -- unless the fall-through is an s_branch that would
    jump over a landmark (a steady block the compiler laid out of line).

The frame has ONE barrier: a pass of the loop is the search and the claim of a frame, barrier A, the ranks and the row of
the frame before, then the rest of the frame up to its filter bank.  Landmarks, in the order a pass meets them: the
ds_read_b128 of the candidate list, ds_min_rtn_u64 (the claim), the s_barrier behind it (barrier A), the row's
global_store_dwordx4 pair, v_div_fixup_f64 (the weights' reciprocal).  They cut the pass into phases:

  chores + search    loop head .. the claim's atomic; and the loop's tail behind the filter bank (the frame's bookkeeping
                     and the closing branch), which runs straight into the next pass's search
  claims             .. behind the claim's own wait and barrier A
  ranks + row        .. behind the row's last store (of the frame before: its deaths are known behind barrier A)
  ageing             .. the end of the seeding block (the last skipped block in front of the reciprocal that stores to the
                     ring in a loop; without one: the last skipped block in front of the reciprocal)
  filter bank        .. behind its last float64 instruction or the ring store (global_store_dwordx4), whichever comes
                     later.  (The source puts a scheduling barrier between the filter bank and what follows, so no
                     instruction of the next search is counted here and none of the filter bank is counted there.)

The report ends with the number of s_barrier on the walked path.

Per phase: VALU (every v_* instruction; the lane moves v_readlane / v_writelane / v_readfirstlane are part of it and listed
again on their own), float64 (v_*_f64, compares included), v_cndmask, lane moves, v_mov, compares, SALU, LDS, VMEM.
The last line, "filter bank, by hand", adds what the round-11 issue's hand count of the parent included beyond the steady
path (the seeding block's tail behind its ring-store loop, the instructions an s_branch jumps over): 242 VALU there.
`census()` returns the same as a dict for tests/test_kernel_hot_path.py.

The round-trip report follows: for every `s_waitcnt lgkmcnt(N)` on the walked path, the youngest scalar load or LDS access
the wave can be waiting for there and how many instructions lie between the two (tests/test_kernel_round_trips.py).
"""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

KERNEL = "_ZN12_GLOBAL__N_17k_batchENS_10BlKernArgsE"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
COND = ("s_cbranch_execz", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_scc0", "s_cbranch_scc1")
STEADY_MARKS = ("ds_read_b128", "ds_min_rtn_u64", "v_div_fixup_f64")
PHASES = ("chores + search", "claims", "ranks + row", "ageing", "filter bank")
COLUMNS = ("valu", "f64", "cndmask", "lane", "mov", "cmp", "salu", "lds", "vmem")


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def listing_of_library(lib):
    """llvm-objdump -d of k_batch out of the library's gfx950 code object; None where the tools or the kernel are missing."""
    objcopy, objdump = _tool("llvm-objcopy"), _tool("llvm-objdump")
    if not objcopy or not objdump or not os.path.exists(lib):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(tmp, "host.so")], check=True,
                       capture_output=True)
        data = open(fat, "rb").read()
        at, k = data.find(BUNDLE_MAGIC), 0
        while at >= 0:
            (n,) = struct.unpack_from("<Q", data, at + len(BUNDLE_MAGIC))
            p = at + len(BUNDLE_MAGIC) + 8
            for _ in range(n):
                off, size, tlen = struct.unpack_from("<QQQ", data, p)
                triple = data[p + 24:p + 24 + tlen].decode()
                p += 24 + tlen
                if triple.endswith("gfx950") and size:
                    path = os.path.join(tmp, f"co{k}.o")
                    k += 1
                    with open(path, "wb") as fh:
                        fh.write(data[at + off:at + off + size])
                    text = subprocess.run([objdump, "-d", f"--disassemble-symbols={KERNEL}", path], check=True,
                                          capture_output=True, text=True).stdout
                    if re.search(r"^[0-9a-f]+ <" + re.escape(KERNEL) + r">:", text, re.M):
                        return text
            at = data.find(BUNDLE_MAGIC, at + 1)
    return None


def parse(text):
    """[(mnemonic, operands, target index or None)] of k_batch, from an objdump listing or from -S output."""
    ins, labels, pending = [], {}, []
    m = re.search(r"^[0-9a-f]+ <" + re.escape(KERNEL) + r">:\n", text, re.M)
    if m:                                   # llvm-objdump: "\tmnemonic operands  // ADDRESS: ENCODING <symbol+0xOFFSET>"
        body = text[m.end():]
        end = re.search(r"^[0-9a-f]+ <[^>]+>:\n", body, re.M)
        body = body[:end.start()] if end else body
        base = None
        for line in body.splitlines():
            mm = re.match(r"\s+([a-z][a-z0-9_]*)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
            if not mm:
                continue
            addr = int(mm.group(3), 16)
            base = addr if base is None else base
            labels[addr - base] = len(ins)
            t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", mm.group(4))
            tgt = int(t.group(1), 16) if t else (0 if re.search(r"<" + re.escape(KERNEL) + r">", mm.group(4)) else None)
            pending.append(tgt if mm.group(1).startswith(("s_cbranch", "s_branch")) else None)
            ins.append((mm.group(1), mm.group(2)))
    else:                                   # -S: the function between its label and .Lfunc_end
        m = re.search(r"^" + re.escape(KERNEL) + r":.*\n", text, re.M)
        if not m:
            raise SystemExit(f"{KERNEL} not found in the listing")
        body = text[m.end():]
        end = re.search(r"^\.Lfunc_end\d+:", body, re.M)
        body = body[:end.start()] if end else body
        for line in body.splitlines():
            line = line.split(";")[0].rstrip()
            lm = re.match(r"^(\.?[A-Za-z_][\w.$]*):\s*$", line)
            if lm:
                labels[lm.group(1)] = len(ins)
                continue
            mm = re.match(r"\s+([a-z][a-z0-9_]*)\s*(.*)$", line)
            if not mm or mm.group(1).startswith("."):
                continue
            pending.append(mm.group(2).strip() if mm.group(1).startswith(("s_cbranch", "s_branch")) else None)
            ins.append((mm.group(1), mm.group(2)))
    return [(op, args, labels.get(t) if t is not None else None) for (op, args), t in zip(ins, pending)]


def _loop_head(ins):
    """The frame loop: the backward branch with the longest reach around the candidate list's ds_read_b128 (the prologue may
    hold a ds_read_b128 of its own -- the first frame's grid header -- with no loop around it)."""
    best = None
    for mark in (i for i, (op, _, _) in enumerate(ins) if op == "ds_read_b128"):
        for i, (op, _, tgt) in enumerate(ins):
            if tgt is not None and tgt <= mark < i and (best is None or i - tgt > best[1] - best[0]):
                best = (tgt, i)
    if best is None:
        raise SystemExit("no loop around ds_read_b128: is this k_batch?")
    return best


def _seat_block(ops):
    """The block at the head of the frame loop that gives up a track wave (batch_link.h): barriers of its own around the
    ring copy, whole entries loaded and stored."""
    return ops.count("s_barrier") >= 3 and "global_load_dwordx4" in ops and "global_store_dwordx4" in ops


def walk(ins):
    """Indices of the steady frame's instructions, and the skipped blocks as (first, one past last)."""
    head, close = _loop_head(ins)
    path, skipped, i, seen = [], [], head, set()
    while i not in seen and i < len(ins):
        seen.add(i)
        op, _, tgt = ins[i]
        path.append(i)
        if i == close:
            break
        if op == "s_branch" and tgt is not None and tgt > i:
            i = tgt
            continue
        if op == "s_cbranch_execnz" and tgt is not None and tgt > i and ins[i + 1][0] == "s_branch":
            over = ins[i + 1][2]         # (a steady block laid out of line: the fall-through would jump over it)
            if over is not None and over > tgt and any(o in STEADY_MARKS for o, _, _ in ins[tgt:over]):
                i = tgt
                continue
        if op in COND and tgt is not None and tgt > i and tgt <= close + 1:
            block = [o for o, _, _ in ins[i + 1:tgt]]
            other_half = skipped and skipped[-1][1] == i - 1 and ins[i - 1][0] in ("s_andn2_saveexec_b64", "s_or_saveexec_b64")
            if other_half:               # (if / else: the first half was skipped as rare, so this half is the steady one)
                i += 1
                continue
            # (the row: two 16-byte stores in straight-line code; a seeding's ring stores sit in a loop)
            row = sum(o == "global_store_dwordx4" for o in block) >= 2 and \
                not any(t is not None and t <= j for j, (_, _, t) in enumerate(ins[i + 1:tgt], i + 1))
            # (what a track requests from memory in every frame -- the ring entries that leave its windows, the claimed
            # detection's box -- sits in short blocks of its own: loads, no barrier, no loop)
            loop = any(t is not None and t <= j for j, (_, _, t) in enumerate(ins[i + 1:tgt], i + 1))
            loads = any(o.startswith("global_load") and not o.startswith("global_load_lds") for o in block) \
                and "s_barrier" not in block and not loop
            # (the candidate list is ONE ds_read_b128 per pass: a block whose only landmark is a second one is the quadrant
            # list of a split cell, a rare path -- per wave and frame; the frame waits for the slowest of its waves.
            # The block is known by that landmark alone, not by what it does: a steady block that gains a second
            # ds_read_b128 of its own would drop out of the census here without notice -- check `skipped blocks` in the
            # report's first line against the last record when the search changes)
            marks = {o for o in block if o in STEADY_MARKS}
            if marks == {"ds_read_b128"} and any(ins[j][0] == "ds_read_b128" for j in path):
                marks = set()
            if _seat_block(block) or (not marks and not row and not loads):
                skipped.append((i + 1, tgt))
                i = tgt
                continue
        i += 1
    return path, skipped


def classify(op):
    out = []
    if op.startswith("v_"):
        out.append("valu")
        if op.startswith("v_cmp"):
            out.append("cmp")
        if "_f64" in op:
            out.append("f64")
        if op.startswith("v_cndmask"):
            out.append("cndmask")
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            out.append("lane")
        if op.startswith("v_mov") or op.startswith("v_accvgpr"):
            out.append("mov")
    elif op.startswith("ds_"):
        out.append("lds")
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        out.append("vmem")
    elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_barrier")):
        out.append("salu")
    return out


def _lgkm_kind(op):
    """'smem' / 'lds' for what s_waitcnt lgkmcnt counts on this path, else None (flat accesses: none in this kernel)."""
    if op.startswith(("s_load_", "s_buffer_load_", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith("ds_"):
        return "lds"
    return None


def round_trips(lines):
    """Every s_waitcnt lgkmcnt(N) of `lines` [(mnemonic, operands)] that can wait for something: the youngest scalar load /
    LDS access it can be waiting for -- the (N + 1)-th youngest still on the books -- and the distance in instructions.
    The books are the wave's own, in program order.  LDS accesses return in order, so a wait for N leaves at most the N
    youngest of them open; scalar loads may return out of order, so a scalar load is credited to a wait for lgkmcnt(0) only
    (which is why the compiler only ever waits for them that way)."""
    out, open_ = [], []
    for k, (op, args) in enumerate(lines):
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", args)
            if not m:
                continue
            n = int(m.group(1))
            lds = [i for i in open_ if _lgkm_kind(lines[i][0]) == "lds"]
            covered = list(open_) if n == 0 else lds[:max(0, len(lds) - n)]
            if covered:
                j = covered[-1]
                out.append({"wait": k, "lgkmcnt": n, "issue": j, "distance": k - j, "op": lines[j][0], "args": lines[j][1],
                            "kind": _lgkm_kind(lines[j][0]), "covers": len(covered),
                            "covered": [(i, _lgkm_kind(lines[i][0])) for i in covered]})
                open_ = [i for i in open_ if i not in covered]
        elif _lgkm_kind(op):
            open_.append(k)
    return out


def _sregs(args):
    """Scalar registers named in an operand string: s7, s[4:5]."""
    out = set()
    for m in re.finditer(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b", args):
        out |= set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}
    return out


def _vregs(args):
    """Vector registers named in an operand string: v7, v[4:7]."""
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", args):
        out |= set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}
    return out


def pending_load_hazards(text):
    """The guard of the kernel's written-out scalar loads (batch_link.h, "Kernel arguments a phase ahead"): an s_load in
    inline assembly hands the compiler registers it believes valid at once, and the matching s_waitcnt lgkmcnt(0) stands in
    another asm statement many instructions later -- so nothing in between may read, copy, spill or overwrite them.
    Checked for EVERY s_load of the kernel (the compiler's own satisfy it by construction), over the whole listing and
    along every path: from the load, through both sides of every conditional branch, to the first s_waitcnt that waits
    for lgkmcnt(0).  Returns [(load index, load text, offending index, offending text)]; empty: clean."""
    ins = parse(text)
    bad = []
    for i, (op, args, _) in enumerate(ins):
        # (the written-out vector loads likewise -- bl_ring_issue16, the ring entries that leave the windows: a 16-byte
        # sc1 load is one the compiler never writes itself; its registers are nobody's up to the first vmcnt(0) wait)
        vector = op == "global_load_dwordx4" and re.search(r"\bsc1\b", args) is not None
        if not vector and not op.startswith(("s_load_", "s_buffer_load_")):
            continue
        regs, done = (_vregs, r"\bvmcnt\(0\)") if vector else (_sregs, r"\blgkmcnt\(0\)")
        dst = regs(args.split(",")[0])
        todo, seen = [i + 1], set()
        while todo:
            j = todo.pop()
            if j in seen or j >= len(ins):
                continue
            seen.add(j)
            o, a, tgt = ins[j]
            if o == "s_waitcnt" and re.search(done, a):
                continue
            if regs(a) & dst:
                bad.append((i, f"{op} {args}", j, f"{o} {a}"))
                continue
            if o == "s_endpgm":
                continue
            if o == "s_branch":
                todo.append(tgt if tgt is not None else j + 1)
                continue
            if o.startswith("s_cbranch") and tgt is not None:
                todo.append(tgt)
            todo.append(j + 1)
    return bad


def census(text):
    ins = parse(text)
    path, skipped = walk(ins)
    pos = {i: k for k, i in enumerate(path)}
    ops = [ins[i][0] for i in path]

    def first(op, start=0):
        return next(k for k in range(start, len(ops)) if ops[k] == op)

    claim = first("ds_min_rtn_u64")
    bar_a = first("s_barrier", claim)
    div = first("v_div_fixup_f64")
    # the row: the first pair of 16-byte stores behind barrier A, and the stores that follow them directly
    row_end = first("global_store_dwordx4", first("global_store_dwordx4", bar_a) + 1) + 1
    while row_end < len(ops) and (ops[row_end].startswith("global_store") or ops[row_end].startswith("s_waitcnt")):
        row_end += 1
    # the filter bank ends behind its last float64 instruction or the ring store
    fb_end = max(k for k in range(div, len(ops)) if "_f64" in ops[k] or ops[k] == "global_store_dwordx4") + 1
    # the seeding block: skipped, in front of the reciprocal, behind barrier A, with a loop that stores ring entries
    before = [(a, b) for a, b in skipped if a - 1 in pos and bar_a < pos[a - 1] < div]
    seeding = [(a, b) for a, b in before
               if any(o == "global_store_dwordx4" for o, _, _ in ins[a:b]) and any(t is not None and t < j + a for j, (_, _, t) in enumerate(ins[a:b]))]
    cut = (seeding or before)[-1] if (seeding or before) else None
    fb = pos[cut[0] - 1] + 1 if cut else bar_a + 1
    if not bar_a < row_end <= fb <= div < fb_end <= len(path):
        raise SystemExit("the walked path does not have the frame's shape: claim, barrier A, row, filter bank")
    bounds = [0, claim, bar_a + 1, row_end, fb, fb_end]
    out = {}
    for name, a, b in zip(PHASES, bounds, bounds[1:]):
        ks = list(range(a, b)) + (list(range(fb_end, len(path))) if name == "chores + search" else [])
        row = dict.fromkeys(COLUMNS, 0)
        row["instructions"] = len(ks)
        for k in ks:
            for c in classify(ops[k]):
                row[c] += 1
        row["ops"] = [ops[k] for k in ks]
        row["lines"] = [ins[path[k]][:2] for k in ks]
        out[name] = row
    # The filter bank as the round-11 issue counted it by hand: from behind the seeding block's ring-store loop (the block's
    # tail, which a steady frame does not run) and without following an s_branch inside the phase.
    extra = []
    if seeding:
        a, b = seeding[-1]
        back = max(j for j in range(a, b) if ins[j][2] is not None and ins[j][2] <= j)
        extra += [ins[j][0] for j in range(back + 1, b)]
    for k in range(fb, fb_end):
        i = path[k]
        if ops[k] == "s_branch" and ins[i][2] is not None and ins[i][2] > i:
            extra += [ins[j][0] for j in range(i + 1, ins[i][2])]
    hand = {c: out["filter bank"][c] for c in COLUMNS}
    hand["instructions"] = out["filter bank"]["instructions"] + len(extra)
    for o in extra:
        for c in classify(o):
            hand[c] += 1
    out["filter bank, by hand"] = hand
    total = dict.fromkeys(COLUMNS, 0)
    for r in (out[name] for name in PHASES):
        for c in COLUMNS:
            total[c] += r[c]
    total["instructions"] = len(path)
    out["frame"] = total
    out["skipped blocks"] = len(skipped)
    out_path = [ins[i][:2] for i in path]
    # the block that gives up a track wave, and what its trigger costs the steady frame: the scalar arithmetic, the compare
    # and the branch between the loop head and the block (everything else there is the frame's own)
    seats = [(a, b) for a, b in skipped if _seat_block([o for o, _, _ in ins[a:b]]) and a - 1 in pos]
    if len(seats) > 1:
        raise SystemExit(f"{len(seats)} skipped blocks have the seat block's landmark: the landmark no longer names one block")
    if seats:
        # the trigger: the scalar chain that ends in the block's branch -- from the branch back, the compare that sets scc
        # and the instructions that write a register the chain reads (the round-up add, the shift); anything else in front
        # of the branch is the frame's own
        seat = seats[0]
        at = pos[seat[0] - 1]
        trig, need = [ops[at]], set()
        for k in range(at - 1, -1, -1):
            op, args = out_path[k]
            if op.startswith("s_cmp_") and len(trig) == 1:
                trig.append(op); need |= _sregs(args)
            elif len(trig) > 1 and op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_cmp_")):
                dst, _, src = args.partition(",")
                if _sregs(dst) & need:
                    trig.append(op); need = (need - _sregs(dst)) | _sregs(src)
        if len(trig) < 2:
            raise SystemExit("no scalar compare in front of the seat block's branch: is this its trigger?")
        out["seat block"] = {"instructions": seat[1] - seat[0], "branch at": at, "trigger": trig[::-1]}
    out["barriers"] = sum(o == "s_barrier" for o in ops)
    out["path"] = [ins[i][:2] for i in path]
    out["marks"] = {"claim": claim, "barrier A": bar_a, "row end": row_end, "filter bank": fb, "filter bank end": fb_end}
    out["kernel instructions"] = len(ins)
    # the round trips of a steady pass: the path walked twice, so that a load issued in the loop's tail meets its wait in
    # the next pass's search; positions are those of the second pass (an issue in the pass before: negative)
    lines, n_path = out["path"], len(path)
    trips = []
    for t in round_trips(lines + lines):
        if t["wait"] >= n_path:
            t = dict(t, wait=t["wait"] - n_path, issue=t["issue"] - n_path, covered=[(i - n_path, k) for i, k in t["covered"]])
            t["phase"] = next(name for name, a, b in zip(PHASES, bounds, bounds[1:]) if a <= t["wait"] < b) \
                if t["wait"] < fb_end else PHASES[0]
            trips.append(t)
    out["round trips"] = trips
    return out


def smem_waits(c):
    """[(wait, issue, distance, text)] of every scalar load of the steady pass, with the wait that first covers it."""
    path = c["path"]
    return [(t["wait"], i, t["wait"] - i, " ".join(path[i])) for t in c["round trips"] for i, kind in t["covered"] if kind == "smem"]


def lds_rounds_before_claim(c):
    """Waits on LDS accesses between the loop head and the claim's atomic that start a round trip of their own: the
    access waited for was issued behind the wait before (the partial waits lgkmcnt(7) .. (0) that take eight reads of ONE
    round one by one count once)."""
    rounds, last = [], -1
    for t in c["round trips"]:
        if 0 <= t["wait"] <= c["marks"]["claim"] and any(kind == "lds" and i > last for i, kind in t["covered"]):
            rounds.append(t["wait"])
            last = t["wait"]
    return rounds


def report_round_trips(c):
    """One line per s_waitcnt lgkmcnt of the steady pass that can wait for something."""
    marks = c["marks"]
    lines = [f"round trips on the steady path (positions from the loop head; claim at {marks['claim']}, barrier A at "
             f"{marks['barrier A']}, filter bank {marks['filter bank']} .. {marks['filter bank end']})",
             f"{'wait at':>8s} {'lgkmcnt':>8s} {'issued':>7s} {'distance':>9s}  {'phase':18s} youngest access it can wait for"]
    for t in c["round trips"]:
        lines.append(f"{t['wait']:8d} {t['lgkmcnt']:8d} {t['issue']:7d} {t['distance']:9d}  {t['phase']:18s} {t['op']} {t['args']}"
                     + (f"   (+{t['covers'] - 1} older)" if t["covers"] > 1 else ""))
    smem = smem_waits(c)
    rounds = lds_rounds_before_claim(c)
    lines.append(f"scalar loads: {len(smem)}, waited for within 8 instructions: {sum(d <= 8 for _, _, d, _ in smem)}; "
                 f"LDS round trips from the loop head to the claim: {len(rounds)} (waits at {rounds})")
    return "\n".join(lines)


def report(c):
    lines = [f"k_batch: {c['kernel instructions']} instructions, steady frame {c['frame']['instructions']}, "
             f"{c['skipped blocks']} guarded blocks skipped",
             f"{'phase':18s}" + "".join(f"{k:>9s}" for k in ("instr",) + COLUMNS)]
    for name in PHASES + ("frame", "filter bank, by hand"):
        r = c[name]
        lead = f"{name:18s}" if len(name) <= 18 else f"{name}\n{'':18s}"
        lines.append(lead + f"{r['instructions']:9d}" + "".join(f"{r[k]:9d}" for k in COLUMNS))
    lines.append(f"s_barrier on the walked path: {c['barriers']}")
    if "seat block" in c:
        sb = c["seat block"]
        lines.append(f"the block that gives up a track wave: {sb['instructions']} instructions, skipped; its trigger adds "
                     f"{len(sb['trigger'])} instructions to \"chores + search\" ({' '.join(sb['trigger'])}), the branch is "
                     f"instruction {sb['branch at']} of the pass")
    return "\n".join(lines)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "ysmr_amd", "csrc", "libysmr_hip.so")
    with open(src, "rb") as fh:
        elf = fh.read(4) == b"\x7fELF"
    text = listing_of_library(src) if elf else open(src).read()
    if text is None:
        raise SystemExit("no gfx950 listing of k_batch: llvm-objcopy / llvm-objdump or the kernel are missing")
    c = census(text)
    print(report(c))
    print()
    print(report_round_trips(c))
    bad = pending_load_hazards(text)
    print(f"scalar loads and written-out 16-byte ring loads whose registers are touched before their wait, whole kernel, every path: {len(bad)}")
    for i, load, j, what in bad:
        print(f"  {load} (instruction {i}): {what} (instruction {j})")
    if bad:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
