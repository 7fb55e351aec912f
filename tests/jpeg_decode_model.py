"""The Motion-JPEG decoder of ``ysmr_mjpeg_decode_batch`` (csrc/mjpeg_decode.hip), written down in NumPy with integer
arithmetic only: the specification the kernels are tested against, byte for byte and status for status.  Its own yardstick
is Pillow (libjpeg-turbo's default decode: the accurate integer IDCT, fancy upsampling, 16-bit colour tables), whose pixels
the fixture ``tests/golden/mjpeg_decode_streams.npz`` records.

Supported: baseline sequential JPEG (SOF0, 8 bit, Huffman), ONE interleaved scan of all components; one component sampled
1 x 1 (``sampling`` 0), or three (ids 1, 2, 3) with luminance sampled 1 x 1, 2 x 1 or 2 x 2 and both chrominances 1 x 1
(``sampling`` 1, 2, 3).  Everything else is flagged: ``UNSUPPORTED`` for what a full decoder could read, ``CORRUPT`` for a
stream that contradicts itself.  A flagged frame's pixels are undefined.

* markers: any number of 0xFF fill bytes before a marker; DQT (8-bit), SOF0, DHT, DRI, SOS are read, APP14 and every other
  SOF flag the frame, all other segments are skipped.  A Huffman table slot 0 or 1 that no DHT defines holds the typical
  table of Annex K.3 (what Motion-JPEG frames leave out);
* entropy data: from the SOS header to the first marker that is not RSTn (0xFF followed by anything but 0x00, 0xFF, 0xD0 ..
  0xD7).  With DRI = Ri > 0 the k-th RST marker must be RST(k mod 8) and there must be ceil(MCUs / Ri) - 1 of them; every
  interval is decoded on its own (DC predictors 0), bounded by its own end: bits beyond it read as 0 and flag the frame;
* IDCT: the accurate integer one (13-bit constants, columns first keeping 2 extra bits, descale by 11 then by 18) in the
  widths libjpeg-turbo's vector code gives it, which is what Pillow runs on every x86-64 and arm64: the dequantised
  coefficient is the product's low 16 bits, sums are 32 bits wide, the first pass's results saturate to 16 bits and the
  samples to -128 .. 127 before + 128.  (Its portable C code, which only runs under JSIMD_FORCENONE=1, keeps 64-bit sums and
  looks the sample up in a table indexed with ``x & 1023``: the same for |x| < 512, a wrap instead of a clamp beyond.  The
  fixture's range-limit stream tells the two apart; the host path delivers the former.);
* upsampling: the "fancy" triangle filters, chroma planes ceil(W / 2) (x ceil(H / 2)) samples, edges as in ``_chroma``;
* colour: 16-bit fixed point, ``R = Y + ((91881 Cr' + 32768) >> 16)``, ``B = Y + ((116130 Cb' + 32768) >> 16)``,
  ``G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16)``, clamped; delivered as B, G, R.
"""
import numpy as np

import jpeg_model as jm

__all__ = ["decode", "UNSUPPORTED", "CORRUPT", "idct_blocks"]

UNSUPPORTED, CORRUPT = 1, 2

#: (horizontal, vertical) sampling factor of the luminance for ``sampling`` 0 .. 3
LUMA_FACTORS = ((1, 1), (1, 1), (2, 1), (2, 2))

_STD = {(0, 0): (jm.DC_LUM_BITS, jm.DC_VALS), (0, 1): (jm.DC_CHR_BITS, jm.DC_VALS),
        (1, 0): (jm.AC_LUM_BITS, jm.AC_LUM_VALS), (1, 1): (jm.AC_CHR_BITS, jm.AC_CHR_VALS)}


class _Flag(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def _derive(bits, vals):
    """{(length, code): symbol} of a table, or CORRUPT if its codes do not fit their lengths (T.81 Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if code >= 1 << length:
                raise _Flag(CORRUPT)
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _headers(data, height, width, sampling):
    """Walk the markers up to the SOS header.  Returns (quantisation tables of the components [nc][64] natural order,
    Huffman tables {(class, slot): {(length, code): symbol}}, (dc slot, ac slot) per component, Ri, start of the entropy data)."""
    n, nc = len(data), (1 if sampling == 0 else 3)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise _Flag(CORRUPT)
    quant, huff, comps, ri, pos = {}, {}, None, 0, 2
    while True:
        if pos >= n or data[pos] != 0xFF:
            raise _Flag(CORRUPT)
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise _Flag(CORRUPT)
        marker = data[pos]
        pos += 1
        if marker == 0x01 or 0xD0 <= marker <= 0xD8:          # stand-alone markers
            continue
        if marker == 0xD9 or marker == 0x00:
            raise _Flag(CORRUPT)
        if pos + 2 > n:
            raise _Flag(CORRUPT)
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2 or pos + length > n:
            raise _Flag(CORRUPT)
        body = data[pos + 2:pos + length]
        if marker == 0xDB:
            at = 0
            while at < len(body):
                if body[at] >> 4:
                    raise _Flag(UNSUPPORTED)                  # 16-bit table
                if (body[at] & 15) > 3 or at + 65 > len(body):
                    raise _Flag(CORRUPT)
                table = np.zeros(64, np.int64)
                table[jm.ZIGZAG] = np.frombuffer(bytes(body[at + 1:at + 65]), np.uint8)
                quant[body[at] & 15] = table
                at += 65
        elif marker == 0xC0:
            if comps is not None:
                raise _Flag(UNSUPPORTED)
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise _Flag(CORRUPT)
            if body[0] != 8 or ((body[1] << 8) | body[2]) != height or ((body[3] << 8) | body[4]) != width or body[5] != nc:
                raise _Flag(UNSUPPORTED)
            comps = [(body[6 + 3 * c], body[7 + 3 * c], body[8 + 3 * c]) for c in range(nc)]
            lh, lv = LUMA_FACTORS[sampling]
            for c, (cid, hv, tq) in enumerate(comps):
                want = ((lh << 4) | lv) if c == 0 else 0x11
                if hv != want or (nc == 3 and cid != c + 1):
                    raise _Flag(UNSUPPORTED)
                if tq > 3:
                    raise _Flag(CORRUPT)
        elif marker == 0xC4:
            at = 0
            while at < len(body):
                tc, th = body[at] >> 4, body[at] & 15
                if tc > 1 or th > 3 or at + 17 > len(body):
                    raise _Flag(CORRUPT)
                bits = list(body[at + 1:at + 17])
                count = sum(bits)
                if count > 256 or at + 17 + count > len(body):
                    raise _Flag(CORRUPT)
                huff[(tc, th)] = _derive(bits, list(body[at + 17:at + 17 + count]))
                at += 17 + count
        elif marker == 0xDD:
            if length != 4:
                raise _Flag(CORRUPT)
            ri = (body[0] << 8) | body[1]
        elif marker == 0xEE or (0xC1 <= marker <= 0xCF and marker != 0xC8):
            raise _Flag(UNSUPPORTED)                          # APP14; any other kind of frame, arithmetic conditioning
        elif marker == 0xDA:
            if comps is None:
                raise _Flag(CORRUPT)
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise _Flag(CORRUPT)
            if body[0] != nc:
                raise _Flag(UNSUPPORTED)
            slots = []
            for c in range(nc):
                if body[1 + 2 * c] != comps[c][0]:
                    raise _Flag(UNSUPPORTED)
                td, ta = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
                if td > 3 or ta > 3:
                    raise _Flag(CORRUPT)
                slots.append((td, ta))
            if body[1 + 2 * nc] != 0 or body[2 + 2 * nc] != 63 or body[3 + 2 * nc] != 0:
                raise _Flag(UNSUPPORTED)
            tables = {}
            for c in range(nc):
                if comps[c][2] not in quant:
                    raise _Flag(CORRUPT)
                for cls, slot in ((0, slots[c][0]), (1, slots[c][1])):
                    if (cls, slot) in huff:
                        tables[(cls, slot)] = huff[(cls, slot)]
                    elif slot < 2:
                        tables[(cls, slot)] = _derive(*_STD[(cls, slot)])
                    else:
                        raise _Flag(CORRUPT)
            return [quant[comps[c][2]] for c in range(nc)], tables, slots, ri, pos + length
        pos += length


def _segments(data, start, n_mcus, ri):
    """[(first byte, end)] of every restart interval of the entropy data that starts at ``start``."""
    n, marks, end, p = len(data), [], len(data), start
    while p + 1 < n:
        if data[p] == 0xFF and data[p + 1] not in (0x00, 0xFF):
            if 0xD0 <= data[p + 1] <= 0xD7:
                marks.append(p)
            else:
                end = p
                break
        p += 1
    n_seg = -(-n_mcus // ri) if ri else 1
    if len(marks) != n_seg - 1:
        raise _Flag(CORRUPT)
    for k, p in enumerate(marks):
        if data[p + 1] != 0xD0 + (k & 7):
            raise _Flag(CORRUPT)
    starts = [start] + [p + 2 for p in marks]
    return list(zip(starts, marks + [end]))


class _Reader:
    """The bits of one interval: 0x00 (after any number of further 0xFF) behind a 0xFF removed; zeros beyond the end."""

    def __init__(self, data, start, end):
        out, p = bytearray(), start
        while p < end:
            b = data[p]
            p += 1
            if b == 0xFF:
                while p < end and data[p] == 0xFF:
                    p += 1
                if p < end and data[p] == 0x00:
                    p += 1
                else:
                    break                                       # (a marker, or the end: nothing more to read)
            out.append(b)
        self.n = 8 * len(out)
        self.v = int.from_bytes(bytes(out), "big") if out else 0
        self.at = 0

    def take(self, k):
        if k == 0:
            return 0
        lo = self.n - self.at - k
        self.at += k
        if lo >= 0:
            return (self.v >> lo) & ((1 << k) - 1)
        return ((self.v << -lo) & ((1 << k) - 1)) if -lo < k else 0

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise _Flag(CORRUPT)

    def value(self, size):
        v = self.take(size)
        return v if v >= 1 << (size - 1) else v - (1 << size) + 1


def _coefficients(data, height, width, sampling, tables, slots, ri, start):
    """Quantised coefficients in natural order, one int64 [block rows, block columns, 64] per component."""
    lh, lv = LUMA_FACTORS[sampling]
    nc = 1 if sampling == 0 else 3
    mx, my = -(-width // (8 * lh)), -(-height // (8 * lv))
    planes = [np.zeros((my * (lv if c == 0 else 1), mx * (lh if c == 0 else 1), 64), np.int64) for c in range(nc)]
    per = ri if ri else mx * my
    for k, (first, end) in enumerate(_segments(data, start, mx * my, ri)):
        bits, pred = _Reader(data, first, end), [0] * nc
        for mcu in range(k * per, min((k + 1) * per, mx * my)):
            for c in range(nc):
                h, v = (lh, lv) if c == 0 else (1, 1)
                dc, ac = tables[(0, slots[c][0])], tables[(1, slots[c][1])]
                for sub in range(h * v):
                    block = planes[c][(mcu // mx) * v + sub // h, (mcu % mx) * h + sub % h]
                    size = bits.symbol(dc)
                    if size > 11:
                        raise _Flag(CORRUPT)
                    if size:
                        pred[c] += bits.value(size)
                    block[0] = pred[c]
                    i = 1
                    while i < 64:
                        rs = bits.symbol(ac)
                        run, size = rs >> 4, rs & 15
                        if size == 0:
                            if run != 15:
                                break
                            i += 16
                            continue
                        i += run
                        if i > 63:
                            raise _Flag(CORRUPT)
                        block[jm.ZIGZAG[i]] = bits.value(size)
                        i += 1
        if bits.at > bits.n:
            raise _Flag(CORRUPT)
    return planes


def _wrap(x, bits):
    """``x`` as a two's-complement number of ``bits`` bits."""
    half = 1 << (bits - 1)
    return ((x + half) & ((1 << bits) - 1)) - half


def _pass(d, shift):
    """One direction of the IDCT over axis -1 of ``d`` (int64 [..., 8]): 32-bit sums, rounded and shifted."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    return _wrap(out + (1 << (shift - 1)), 32) >> shift


def idct_blocks(coef, quant):
    """uint8-valued samples [..., 8, 8] of quantised coefficients [..., 64] (natural order) and their table [64]."""
    d = _wrap(coef * quant, 16).reshape(coef.shape[:-1] + (8, 8))
    ws = np.swapaxes(_pass(np.swapaxes(d, -1, -2), 11), -1, -2)          # columns first
    return np.clip(_pass(np.clip(ws, -32768, 32767), 18), -128, 127) + 128


def _plane(coef, quant):
    rows, cols = coef.shape[:2]
    return idct_blocks(coef, quant).transpose(0, 2, 1, 3).reshape(8 * rows, 8 * cols)


def _chroma(plane, height, width, sampling):
    """A chrominance plane at full size.  The plane is the decoded one, whole blocks wide and high; only its first
    ceil(W / 2) columns (and ceil(H / 2) rows) are the component, and the filters' ends are set by those numbers."""
    if sampling == 1:
        return plane[:height, :width]
    cw = -(-width // 2)
    x = np.arange(width)
    j, odd = x >> 1, (x & 1).astype(bool)
    other = np.where(odd, j + 1, j - 1)
    # (the first sample and the last of 2 cw are single-sided; a one-sample component still reads its right neighbour)
    end = (x == 0) | ((x == 2 * cw - 1) & (cw > 1))
    other = np.where(end, j, other)
    if sampling == 2:
        p = plane[:height]
        full = np.where(odd, (3 * p[:, j] + p[:, other] + 2) >> 2, (3 * p[:, j] + p[:, other] + 1) >> 2)
        return np.where(end, p[:, j], full)
    ch = -(-height // 2)
    y = np.arange(height)
    i = y >> 1
    near = np.clip(np.where(y & 1, i + 1, i - 1), 0, ch - 1)
    s = 3 * plane[i] + plane[near]                                       # column sums [H, plane width]
    full = np.where(odd, (3 * s[:, j] + s[:, other] + 7) >> 4, (3 * s[:, j] + s[:, other] + 8) >> 4)
    return np.where(end, np.where(odd, (4 * s[:, j] + 7) >> 4, (4 * s[:, j] + 8) >> 4), full)


def decode(jpeg_bytes, height, width, sampling):
    """(status, uint8 [H, W] for ``sampling`` 0, else [H, W, 3] as B, G, R).  Pixels of a flagged frame are zero here and
    undefined on the device."""
    if sampling not in (0, 1, 2, 3):
        raise ValueError("sampling must be 0 .. 3, got {}".format(sampling))
    data = bytes(jpeg_bytes)
    shape = (height, width) if sampling == 0 else (height, width, 3)
    try:
        quant, tables, slots, ri, start = _headers(data, height, width, sampling)
        coef = _coefficients(data, height, width, sampling, tables, slots, ri, start)
    except _Flag as flag:
        return flag.status, np.zeros(shape, np.uint8)
    luma = _plane(coef[0], quant[0])[:height, :width]
    if sampling == 0:
        return 0, luma.astype(np.uint8)
    cb = _chroma(_plane(coef[1], quant[1]), height, width, sampling) - 128
    cr = _chroma(_plane(coef[2], quant[2]), height, width, sampling) - 128
    r = luma + ((91881 * cr + 32768) >> 16)
    g = luma + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = luma + ((116130 * cb + 32768) >> 16)
    return 0, np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)
