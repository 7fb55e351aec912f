"""The Motion-JPEG stream of ``ysmr_mjpeg_batch`` (csrc/mjpeg.hip), written down in NumPy with integer arithmetic only: the
specification the kernels are tested against, byte for byte.

One frame is a baseline sequential JPEG (ITU-T T.81, SOF0): 8-bit Y, Cb, Cr, all sampled 1 x 1; SOI, APP0 ``AVI1``, one DQT
with tables 0 and 1, SOF0, four DHT (the typical tables of Annex K.3), DRI, SOS, entropy-coded data, EOI.  One MCU row is
one restart interval.

* colour: JFIF BT.601 full range in 16-bit fixed point, ``(c0 * R + c1 * G + c2 * B + half) >> 16``, half = 32768 for Y and
  32767 for Cb, Cr, which then get + 128 (so that B = 255 alone stays at 255), clamped to 0 .. 255;
* edges: the last column / row repeated up to a multiple of 8;
* forward DCT: the definition of T.81 A.3.3 as two matrix products with the matrix ``round(2 ** 16 * c(u) / 2 *
  cos((2 x + 1) u pi / 16))`` held as integers (``DCT_MATRIX``, entries below 2 ** 15).  The first product (along a row)
  is kept whole: a row of the matrix sums to at most 185360 in absolute values (the first row, 8 * 23170), so it is at
  most 128 * 185360 < 2 ** 25.  The second is a 64-bit sum (below 2 ** 43), scaled by 2 ** 32, and is rounded to 12
  fraction bits, ``(sum + 2 ** 19) >> 20``: at most 1024 * 4096 plus the matrix's rounding, far inside 32 bits;
* quantisation: ``sign(c) * ((|c| + (q << 11)) // (q << 12))`` -- half away from zero --, AC clamped to +-1023 and DC to
  [-1024, 1023].
"""
import math

import numpy as np

__all__ = ["encode", "encode_info", "chunk", "quant_tables", "header", "DCT_MATRIX", "ZIGZAG"]

# ---- tables of the standard ------------------------------------------------------------------------------------------
# Annex K.1 / K.2, in natural (row-major) order
K1_LUMINANCE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
K1_CHROMINANCE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] +
    [99] * 32, dtype=np.int64)


def _zigzag():
    """ZIGZAG[k] = natural index (8 * row + column) of the k-th coefficient of the zigzag sequence (T.81 figure 5)."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, dtype=np.int64)


ZIGZAG = _zigzag()

# Annex K.3: BITS (codes per length 1 .. 16) and HUFFVAL of the four typical tables
DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
    0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
    0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
    0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]


def _codes(bits, vals):
    """{symbol: (code, length)} by T.81 Annex C: codes of one length count up, a longer length starts at twice the next."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return table


DC_CODES = (_codes(DC_LUM_BITS, DC_VALS), _codes(DC_CHR_BITS, DC_VALS))
AC_CODES = (_codes(AC_LUM_BITS, AC_LUM_VALS), _codes(AC_CHR_BITS, AC_CHR_VALS))

#: DCT_MATRIX[u, x] = round(2 ** 16 * c(u) / 2 * cos((2 x + 1) u pi / 16)), c(0) = 1 / sqrt(2), c(u) = 1  (T.81 A.3.3)
DCT_MATRIX = np.array([[int(math.floor(65536 * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) + 0.5))
                        for x in range(8)] for u in range(8)], dtype=np.int64)


def quant_tables(quality):
    """(luminance, chrominance) in natural order for quality 1 .. 100."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be 1 .. 100, got {}".format(quality))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (K1_LUMINANCE, K1_CHROMINANCE))


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(height, width, quality):
    """Everything from SOI up to and including the SOS header."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"AVI1" + bytes(10))
    out += _segment(0xDB, bytes([0]) + bytes(ql[ZIGZAG].astype(np.uint8)) + bytes([1]) + bytes(qc[ZIGZAG].astype(np.uint8)))
    out += _segment(0xC0, bytes([8]) + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") +
                    bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS),
                              (0x01, DC_CHR_BITS, DC_VALS), (0x11, AC_CHR_BITS, AC_CHR_VALS)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, ((int(width) + 7) // 8).to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def ycbcr(bgr):
    """int64 [H, W, 3] (Y, Cb, Cr) of a uint8 [H, W, 3] (B, G, R) image."""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11059 * r - 21709 * g + 32768 * b + 32767) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32767) >> 16) + 128
    return np.clip(np.stack([y, cb, cr], axis=-1), 0, 255)


def coefficients(bgr, quality):
    """Quantised coefficients in zigzag order, int64 [rows, columns, 3, 64] (MCU row, MCU column, component)."""
    h, w = bgr.shape[:2]
    h8, w8 = (h + 7) // 8, (w + 7) // 8
    ycc = ycbcr(bgr)
    ycc = ycc[np.minimum(np.arange(8 * h8), h - 1)][:, np.minimum(np.arange(8 * w8), w - 1)] - 128
    blocks = ycc.reshape(h8, 8, w8, 8, 3).transpose(0, 2, 4, 1, 3)                   # [row, column, component, y, x]
    rows = np.einsum("ux,rkcyx->rkcyu", DCT_MATRIX, blocks)                          # along x: [.., y, u], scaled 2 ** 16
    full = np.einsum("vy,rkcyu->rkcvu", DCT_MATRIX, rows)                            # along y: [.., v, u], scaled 2 ** 32
    assert np.abs(DCT_MATRIX).sum(axis=1).max() == 185360 and np.abs(rows).max() < 1 << 25
    full = (full + (1 << 19)) >> 20                                                   # 12 fraction bits
    ql, qc = quant_tables(quality)
    q = np.stack([ql, qc, qc]).reshape(3, 8, 8)
    quant = np.sign(full) * ((np.abs(full) + (q << 11)) // (q << 12))
    quant = quant.reshape(h8, w8, 3, 64)[..., ZIGZAG]
    quant[..., 0] = np.clip(quant[..., 0], -1024, 1023)
    quant[..., 1:] = np.clip(quant[..., 1:], -1023, 1023)
    return quant


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def bytes_padded(self):
        pad = -self.n % 8
        return ((self.acc << pad) | ((1 << pad) - 1)).to_bytes((self.n + pad) // 8, "big")


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, size):
    v = int(v)
    return v if v >= 0 else v + (1 << size) - 1


def encode_info(bgr, quality):
    """(stream, counters): counters = {'stuffed': bytes 0x00 inserted after a 0xFF, 'zrl': ZRL codes, 'max_category': the
    largest size category coded (DC differences included), 'max_dc_category', 'interval_bytes': bytes of every restart interval
    after stuffing, without its RST marker}."""
    bgr = np.asarray(bgr)
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError("encode needs a uint8 [H, W, 3] image")
    h, w = bgr.shape[:2]
    coef = coefficients(bgr, quality)
    out = bytearray(header(h, w, quality))
    info = {"stuffed": 0, "zrl": 0, "max_category": 0, "max_dc_category": 0, "interval_bytes": []}
    for row in range(coef.shape[0]):
        bits, pred = _Bits(), [0, 0, 0]
        for col in range(coef.shape[1]):
            for comp in range(3):
                block, t = coef[row, col, comp], min(comp, 1)
                diff = int(block[0]) - pred[comp]
                pred[comp] = int(block[0])
                size = _category(diff)
                info["max_dc_category"] = max(info["max_dc_category"], size)
                info["max_category"] = max(info["max_category"], size)
                bits.put(*DC_CODES[t][size])
                if size:
                    bits.put(_value_bits(diff, size), size)
                run = 0
                for k in range(1, 64):
                    v = int(block[k])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*AC_CODES[t][0xF0])
                        info["zrl"] += 1
                        run -= 16
                    size = _category(v)
                    info["max_category"] = max(info["max_category"], size)
                    bits.put(*AC_CODES[t][(run << 4) | size])
                    bits.put(_value_bits(v, size), size)
                    run = 0
                if run:
                    bits.put(*AC_CODES[t][0x00])
        raw = bits.bytes_padded()
        stuffed = raw.replace(b"\xff", b"\xff\x00")
        info["stuffed"] += len(stuffed) - len(raw)
        info["interval_bytes"].append(len(stuffed))
        out += stuffed
        if row + 1 < coef.shape[0]:
            out += bytes([0xFF, 0xD0 + row % 8])
    out += b"\xff\xd9"
    return bytes(out), info


def encode(bgr, quality):
    """The JPEG of a uint8 [H, W, 3] (B, G, R) image."""
    return encode_info(bgr, quality)[0]


def chunk(jpeg):
    """The AVI chunk of one frame: '00dc', the payload size, the JPEG, a zero byte if the size is odd."""
    return b"00dc" + len(jpeg).to_bytes(4, "little") + jpeg + bytes(len(jpeg) & 1)
