"""The entropy decode of ``ysmr_mjpeg_decode_batch_sync`` for a frame WITHOUT restart markers (csrc/mjpeg_decode.hip:
k_mjd_destuff, k_mjd_sync, k_mjd_dc), written down in plain Python: the specification of its intermediate results --
coefficients, status and the number of rounds every pass took.  ``jpeg_decode_model`` stays the specification of the pixels,
and its serial ``_coefficients`` is what this one must equal for every stream.

* the reader's rules are ``jpeg_decode_model._Reader``'s, applied ONCE: the data without stuffing and fill bytes, up to the
  marker that ends it.  Behind that a position is a bit number, bits behind the end are zeros;
* the data is cut into subsequences of ``subsequence_bytes``; a pass takes ``subsequences_per_pass`` consecutive ones, a lane
  each.  A decoder's state between two symbols (a symbol is a Huffman code with the value bits behind it) is
  (bit position, block inside the MCU, zigzag index, error);
* lane 0 of a pass starts from the TRUE state (the frame's start, or the exit state of the pass before), every other lane at
  its first bit, expecting the DC symbol of block 0.  A round: every lane whose entry state changed decodes the symbols that
  START inside its subsequence, stores nothing, and publishes its exit state and the blocks it completed; then every lane
  takes its predecessor's exit state for its entry.  The pass's rounds end when NO entry state changed -- after round r the
  first r lanes hold true states, so that happens after ``subsequences_per_pass`` rounds at the latest, and then every entry
  state is the true one.  A code that no table holds, a DC category above 11 or an index past 63 is an exit state (error) like
  any other: it flags nothing, and the successor of a lane that left with it keeps to its own assumed state -- the error of
  one wrong guess must not silence the lanes behind it;
* the write pass: blocks completed before a lane = an exclusive sum; every lane decodes once more from its true state and
  stores, DC as the DIFFERENCE, up to the frame's last block.  Only here the status is decided: CORRUPT for an error inside
  the frame's blocks, for bits of them beyond the data's end, and for data that ends before the last block;
* DC: prefix sums per component over the blocks in scan order.
"""
import numpy as np

import jpeg_decode_model as dm
import jpeg_model as jm

__all__ = ["decode", "coefficients", "destuffed"]


def destuffed(data, start, end):
    """The bytes ``jpeg_decode_model._Reader`` makes its bits of."""
    r = dm._Reader(data, start, end)
    return r.v.to_bytes(r.n // 8, "big") if r.n else b""


class _Bits:
    def __init__(self, data):
        self.n = 8 * len(data)
        self.data = bytes(data) + bytes(8)

    def peek(self, pos, k):
        """k <= 32 bits from bit ``pos`` on; zeros behind the end."""
        at = pos >> 3
        if at >= len(self.data) - 8:
            return 0
        word = int.from_bytes(self.data[at:at + 8], "big")
        return (word >> (64 - (pos & 7) - k)) & ((1 << k) - 1)


def _run(bits, tables, slots, luma, per_mcu, state, stop, store=None):
    """The symbols that start before bit ``stop`` from ``state`` = (pos, k, i, error) on -> (exit state, blocks completed).
    ``store``: None, or (blocks completed before, blocks of the frame, function(block number, k, zigzag index, value)); the
    third result then tells whether the frame is damaged."""
    pos, k, i, error = state
    done = 0
    before, total, put = store if store else (0, None, None)
    ended = store is not None and before >= total
    while pos < stop and not error and not ended:
        c = 0 if k < luma else k - luma + 1
        table = tables[(0, slots[c][0])] if i == 0 else tables[(1, slots[c][1])]
        sym, length, ahead = None, 0, bits.peek(pos, 32)                   # (a code and its value bits: 31 bits at most)
        for length in range(1, 17):
            sym = table.get((length, ahead >> (32 - length)))
            if sym is not None:
                break
        if sym is None or (i == 0 and sym > 11):
            error = True
            break
        size, run = sym & 15, (0 if i == 0 else sym >> 4)
        if i > 0 and size == 0:
            pos += length
            i += 16
            complete = run != 15 or i > 63
        else:
            i += run
            if i > 63:
                error = True
                break
            if put:
                v = (ahead >> (32 - length - size)) & ((1 << size) - 1)
                put(before + done, k, i, (v if v >= 1 << (size - 1) else v - (1 << size) + 1) if size else 0)
            pos += length + size
            i += 1
            complete = i == 64
        if complete:
            i, k, done = 0, (k + 1) % per_mcu, done + 1
            if store is not None and before + done == total:
                ended = True
    damaged = store is not None and before < total and (error or (ended and pos > bits.n))
    return (pos, k, i, error), done, damaged


def coefficients(data, height, width, sampling, tables, slots, start, subsequence_bytes, subsequences_per_pass):
    """(planes as ``jpeg_decode_model._coefficients`` returns them, status, [rounds of every pass]) of a frame without a
    restart interval whose headers ``jpeg_decode_model._headers`` read.  The planes of a flagged frame are undefined."""
    lh, lv = dm.LUMA_FACTORS[sampling]
    nc = 1 if sampling == 0 else 3
    mx, my = -(-width // (8 * lh)), -(-height // (8 * lv))
    luma, per_mcu = lh * lv, (1 if nc == 1 else lh * lv + 2)
    total = mx * my * per_mcu
    planes = [np.zeros((my * (lv if c == 0 else 1), mx * (lh if c == 0 else 1), 64), np.int64) for c in range(nc)]
    try:
        (first, end), = dm._segments(data, start, mx * my, 0)              # (an RSTn in a frame without DRI flags it)
    except dm._Flag as flag:
        return planes, flag.status, []
    bits = _Bits(destuffed(data, first, end))
    sub_bits, per_pass = 8 * subsequence_bytes, subsequences_per_pass
    nsub = -(-(bits.n // 8) // subsequence_bytes)
    scan = [[] for _ in range(nc)]                                          # the blocks of a component in scan order

    def put(number, k, i, value):
        mcu, c = number // per_mcu, (0 if k < luma else k - luma + 1)
        h = lh if c == 0 else 1
        sub = k if c == 0 else 0
        row, col = (mcu // mx) * (lv if c == 0 else 1) + sub // h, (mcu % mx) * h + sub % h
        assert number < total and i < 64
        planes[c][row, col, jm.ZIGZAG[i]] = value

    true, blocks_done, corrupt, rounds = (0, 0, 0, False), 0, False, []
    for s0 in range(0, nsub, per_pass):
        if blocks_done >= total or true[3]:
            break
        lanes = min(per_pass, nsub - s0)
        stops = [min((s0 + j + 1) * sub_bits, bits.n) for j in range(lanes)]
        assumed = [((s0 + j) * sub_bits, 0, 0, False) for j in range(lanes)]
        entry = [true] + assumed[1:]
        was, left, done, count = [None] * lanes, [None] * lanes, [0] * lanes, 0
        changed = list(range(lanes))                                         # the lanes whose entry state changed
        while changed:
            count += 1
            for j in changed:
                left[j], done[j], _ = _run(bits, tables, slots, luma, per_mcu, entry[j], stops[j])
                was[j] = entry[j]
            # (only the successor of a lane that decoded can find another entry state; a predecessor that met an error has
            # nothing to hand on, and its successor keeps to its assumed state)
            for j in changed:
                if j + 1 < lanes:
                    entry[j + 1] = assumed[j + 1] if left[j][3] else left[j]
            changed = [j + 1 for j in changed if j + 1 < lanes and entry[j + 1] != was[j + 1]]
        rounds.append(count)
        before = blocks_done
        for j in range(lanes):
            state, again, damaged = _run(bits, tables, slots, luma, per_mcu, entry[j], stops[j], (before, total, put))
            corrupt = corrupt or damaged
            before += done[j]
        true, blocks_done = left[-1], before
        if corrupt:
            break
    if blocks_done < total:
        corrupt = True
    # DC: the differences summed per component in scan order
    for mcu in range(mx * my):
        for c in range(nc):
            h, v = (lh, lv) if c == 0 else (1, 1)
            for sub in range(h * v):
                scan[c].append(((mcu // mx) * v + sub // h, (mcu % mx) * h + sub % h))
    for c in range(nc):
        rows, cols = np.array(scan[c]).T
        planes[c][rows, cols, 0] = np.cumsum(planes[c][rows, cols, 0])
    return planes, (dm.CORRUPT if corrupt else 0), rounds


def decode(jpeg_bytes, height, width, sampling, subsequence_bytes, subsequences_per_pass):
    """(planes, status, rounds per pass) of a whole stream; a stream WITH a restart interval is not this model's
    (``ValueError``), one whose headers are flagged returns their status."""
    data = bytes(jpeg_bytes)
    try:
        _, tables, slots, ri, start = dm._headers(data, height, width, sampling)
    except dm._Flag as flag:
        return None, flag.status, []
    if ri:
        raise ValueError("a stream with a restart interval is decoded interval by interval")
    return coefficients(data, height, width, sampling, tables, slots, start, subsequence_bytes, subsequences_per_pass)
