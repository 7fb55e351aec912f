"""The Motion-JPEG stream of ``ysmr_mjpeg_encode_batch`` (csrc/mjpeg.hip), written down in NumPy with integer arithmetic
only: ``encode`` and ``chunk`` are the definition of that entry's bytes.  Tables, DCT matrix, colour and quantisation are
those of tests/jpeg_model.py, and ``encode(f, q, 1, 0)`` is ``jpeg_model.encode(f, q)`` byte for byte.

``sampling`` (the codes of the decoder): 1 = 4:4:4, 2 = 4:2:2, 3 = 4:2:0 -- the luminance is sampled h x v = 1 x 1, 2 x 1 or
2 x 2, Cb and Cr 1 x 1.

* the MCU is 8 h x 8 v pixels; the last column / row is repeated up to a multiple of it; an MCU's blocks are its h v
  luminance blocks row by row, then Cb, then Cr (T.81 A.2.3); one MCU row is one restart interval, DRI = ceil(W / 8 h); the
  DC prediction runs per component through the interval, so inside an MCU a luminance block predicts from the one before it;
* downsampling is libjpeg's, on the clamped 0 .. 255 Cb / Cr samples of the padded frame, before the level shift: 2 x 1 by
  ``(a + b + bias) >> 1`` with bias 0, 1, 0, 1, ... along the output row, 2 x 2 by ``(a + b + c + d + bias) >> 2`` with bias
  1, 2, 1, 2, ...;
* ``huffman`` 0: the typical tables of Annex K.3.  1: four tables (DC and AC, luminance and chrominance) built from the
  frame's own symbol counts, ZRL and EOB included.  The code lengths are ``png_dynamic_model.code_lengths`` -- Huffman's tree
  by two queues, the leaf on a tie; lengths beyond the limit repaired; the lengths handed out from the shortest on to the
  symbols in descending order of (count, index) -- with a limit of 16 bits over the alphabet [pseudo-symbol, symbol 0,
  symbol 1, ...]: the pseudo-symbol of T.81 K.2 has the count 1 and the index 0, so it is the lightest of all, is given a
  longest code, and is then left out, which leaves the last code of that length -- all 1-bits -- unused.  Codes are canonical
  (Annex C): by length, then by symbol.  A DHT segment lists only the symbols the frame uses.
"""
import numpy as np

import jpeg_model as jm
from png_dynamic_model import code_lengths

__all__ = ["encode", "encode_info", "chunk", "planes", "coefficients", "build_table", "FACTORS"]

#: (h, v) of the luminance for ``sampling`` 1 .. 3
FACTORS = {1: (1, 1), 2: (2, 1), 3: (2, 2)}

chunk = jm.chunk


def planes(bgr, sampling):
    """(Y, Cb, Cr) as int64 planes of the padded frame, values 0 .. 255: Y [8 v rows, 8 h cols], Cb / Cr [8 rows, 8 cols]
    with (rows, cols) the frame in MCUs."""
    h, v = FACTORS[sampling]
    height, width = bgr.shape[:2]
    rows, cols = -(-height // (8 * v)), -(-width // (8 * h))
    ycc = jm.ycbcr(bgr)
    ycc = ycc[np.minimum(np.arange(8 * v * rows), height - 1)][:, np.minimum(np.arange(8 * h * cols), width - 1)]
    y, chroma = ycc[..., 0], ycc[..., 1:]
    if sampling == 2:
        bias = (np.arange(8 * cols) & 1)[None, :, None]
        chroma = (chroma[:, 0::2] + chroma[:, 1::2] + bias) >> 1
    elif sampling == 3:
        bias = (1 + (np.arange(8 * cols) & 1))[None, :, None]
        chroma = (chroma[0::2, 0::2] + chroma[0::2, 1::2] + chroma[1::2, 0::2] + chroma[1::2, 1::2] + bias) >> 2
    return y, chroma[..., 0], chroma[..., 1]


def _quantised(plane, q):
    """Quantised coefficients in zigzag order [block rows, block cols, 64] of a plane of whole blocks (values 0 .. 255)."""
    rows, cols = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = (plane - 128).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)             # [row, column, y, x]
    along_x = np.einsum("ux,rkyx->rkyu", jm.DCT_MATRIX, blocks)
    full = np.einsum("vy,rkyu->rkvu", jm.DCT_MATRIX, along_x)
    full = (full + (1 << 19)) >> 20
    q = q.reshape(8, 8)
    quant = np.sign(full) * ((np.abs(full) + (q << 11)) // (q << 12))
    quant = quant.reshape(rows, cols, 64)[..., jm.ZIGZAG]
    quant[..., 0] = np.clip(quant[..., 0], -1024, 1023)
    quant[..., 1:] = np.clip(quant[..., 1:], -1023, 1023)
    return quant


def coefficients(bgr, quality, sampling):
    """The quantised coefficients in zigzag order, one int64 [block rows, block cols, 64] per component."""
    ql, qc = jm.quant_tables(quality)
    y, cb, cr = planes(bgr, sampling)
    return _quantised(y, ql), _quantised(cb, qc), _quantised(cr, qc)


def _symbols(block, pred):
    """[(class 0 DC / 1 AC, symbol, value, size)] of one block."""
    diff = int(block[0]) - pred
    size = jm._category(diff)
    out, run = [(0, size, diff, size)], 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        size = jm._category(v)
        out.append((1, (run << 4) | size, v, size))
        run = 0
    if run:
        out.append((1, 0x00, 0, 0))
    return out


def _scan(coef, sampling):
    """The frame's symbols in the order of the scan: [interval][(table 0 luminance / 1 chrominance, class, symbol, value,
    size)]."""
    h, v = FACTORS[sampling]
    rows, cols = coef[1].shape[:2]
    intervals = []
    for r in range(rows):
        pred, out = [0, 0, 0], []
        for c in range(cols):
            order = [(0, v * r + k // h, h * c + k % h) for k in range(h * v)] + [(1, r, c), (2, r, c)]
            for comp, br, bc in order:
                block = coef[comp][br, bc]
                out += [(min(comp, 1),) + s for s in _symbols(block, pred[comp])]
                pred[comp] = int(block[0])
        intervals.append(out)
    return intervals


def build_table(counts):
    """(BITS [16], HUFFVAL) of the table built from ``counts`` (count per symbol value; at least one is used)."""
    counts = [int(c) for c in counts]
    lengths = code_lengths([1] + counts, 16)[1:]                  # the pseudo-symbol first: the lightest, so a longest code
    vals = sorted((s for s in range(len(counts)) if lengths[s]), key=lambda s: (lengths[s], s))
    bits = [sum(1 for s in vals if lengths[s] == n) for n in range(1, 17)]
    assert all((counts[s] > 0) == (lengths[s] > 0) for s in range(len(counts)))
    return bits, vals


def header(height, width, quality, sampling, tables):
    """Everything from SOI up to and including the SOS header; ``tables``: (BITS, HUFFVAL) of DC luminance, AC luminance,
    DC chrominance, AC chrominance."""
    h, v = FACTORS[sampling]
    ql, qc = jm.quant_tables(quality)
    out = b"\xff\xd8" + jm._segment(0xE0, b"AVI1" + bytes(10))
    out += jm._segment(0xDB, bytes([0]) + bytes(ql[jm.ZIGZAG].astype(np.uint8)) + bytes([1]) + bytes(qc[jm.ZIGZAG].astype(np.uint8)))
    out += jm._segment(0xC0, bytes([8]) + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") +
                       bytes([3, 1, (h << 4) | v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), tables):
        out += jm._segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += jm._segment(0xDD, (-(-int(width) // (8 * h))).to_bytes(2, "big"))
    out += jm._segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


_STANDARD = ((jm.DC_LUM_BITS, jm.DC_VALS), (jm.AC_LUM_BITS, jm.AC_LUM_VALS), (jm.DC_CHR_BITS, jm.DC_VALS), (jm.AC_CHR_BITS, jm.AC_CHR_VALS))


def encode_info(bgr, quality, sampling=1, huffman=0):
    """(stream, info): info = {'tables': the four (BITS, HUFFVAL) in the order of the DHT segments, 'counts': the four symbol
    histograms [256], 'coefficients': ``coefficients``' result, 'data_bits': bits of entropy-coded data before padding}."""
    bgr = np.asarray(bgr)
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError("encode needs a uint8 [H, W, 3] image")
    if sampling not in FACTORS or huffman not in (0, 1):
        raise ValueError("sampling must be 1, 2 or 3 and huffman 0 or 1, got {!r} and {!r}".format(sampling, huffman))
    height, width = bgr.shape[:2]
    coef = coefficients(bgr, quality, sampling)
    intervals = _scan(coef, sampling)
    counts = [[0] * 256 for _ in range(4)]                         # DC lum, AC lum, DC chr, AC chr
    for interval in intervals:
        for t, cls, sym, _v, _size in interval:
            counts[2 * t + cls][sym] += 1
    tables = tuple(build_table(c) for c in counts) if huffman else _STANDARD
    codes = [jm._codes(list(bits), list(vals)) for bits, vals in tables]
    out = bytearray(header(height, width, quality, sampling, tables))
    data_bits = 0
    for row, interval in enumerate(intervals):
        bits = jm._Bits()
        for t, cls, sym, v, size in interval:
            bits.put(*codes[2 * t + cls][sym])
            if size:
                bits.put(jm._value_bits(v, size), size)
        data_bits += bits.n
        out += bits.bytes_padded().replace(b"\xff", b"\xff\x00")
        if row + 1 < len(intervals):
            out += bytes([0xFF, 0xD0 + row % 8])
    out += b"\xff\xd9"
    return bytes(out), {"tables": tables, "counts": counts, "coefficients": coef, "data_bits": data_bits}


def encode(bgr, quality, sampling=1, huffman=0):
    """The JPEG of a uint8 [H, W, 3] (B, G, R) image."""
    return encode_info(bgr, quality, sampling, huffman)[0]
