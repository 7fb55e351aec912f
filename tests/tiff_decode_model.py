"""The specification of ``ysmr_tiff_decode_batch`` (csrc/tiff_decode.hip) in NumPy / Python: what a strip's body decodes to, byte for
byte, and which status bits a frame gets.  LZW follows TIFF 6.0 as libtiff decodes it; where a stream is damaged the model says
where decoding stops, and the kernels equal it in pixels and in status.

A frame is decoded strip by strip into its own ``rows * W * channels`` bytes; afterwards predictor 2 (a running sum mod 256 along a
row, per channel), photometric 0 (inverted) and 2 (R, G, B -> B, G, R) are applied to the whole frame."""
import numpy as np

BAD_CODE, SHORT, OVERRUN, OLD_LZW, TABLE = 1, 2, 4, 8, 16        # YSMR_TIFFD_*
CLEAR, EOI, FIRST = 256, 257, 258
MAX_RUN = 4095 - 257              # data codes after a Clear that may add an entry: the last one adds entry 4095

NONE, LZW, PACKBITS = 1, 5, 32773


def lzw_decode(body, need, stats=None):
    """(status, bytes written) of one strip: ``need`` bytes are wanted.  ``stats`` (a dict) receives what the stream was made of:
    codes, clears, kwkwk, widest, longest."""
    body = bytes(body)
    out = bytearray()
    if len(body) >= 2 and body[0] == 0 and body[1] & 1:
        return OLD_LZW, bytes(out)
    total_bits = 8 * len(body)
    bitpos, nbits, n = 0, 9, 0
    starts = []                   # where the output of the i-th data code since the Clear begins
    codes = clears = kwkwk = longest = 0
    widest = 9
    status = 0
    while len(out) < need:
        if bitpos + nbits > total_bits:
            break
        at, bit = bitpos >> 3, bitpos & 7
        window = int.from_bytes(body[at:at + 3].ljust(3, b"\0"), "big")
        code = (window >> (24 - bit - nbits)) & ((1 << nbits) - 1)
        bitpos += nbits
        codes += 1
        widest = max(widest, nbits)
        if code == EOI:
            break
        if code == CLEAR:
            n, nbits, starts = 0, 9, []
            clears += 1
            continue
        i = code - FIRST
        if i >= n or n > MAX_RUN:
            status = BAD_CODE
            break
        starts.append(len(out))
        if code < 256:
            out.append(code)
        else:
            begin = starts[i]
            length = starts[i + 1] - begin + 1
            if i == n - 1:                       # the code that is the next free entry: its last byte is its first
                kwkwk += 1
                string = bytes(out[begin:begin + length - 1]) + bytes(out[begin:begin + 1])
            else:
                string = bytes(out[begin:begin + length])
            longest = max(longest, length)
            out += string[:need - len(out)]
        n += 1
        free = FIRST - 1 + n
        nbits = 12 if free >= 2047 else 11 if free >= 1023 else 10 if free >= 511 else 9
    if status == 0 and len(out) < need:
        status = SHORT
    if stats is not None:
        stats.update(codes=codes, clears=clears, kwkwk=kwkwk, widest=widest, longest=longest)
    return status, bytes(out)


def packbits_decode(body, need):
    body = bytes(body)
    out = bytearray()
    at = 0
    while len(out) < need:
        if at >= len(body):
            return SHORT, bytes(out)
        h = body[at] - 256 if body[at] > 127 else body[at]
        at += 1
        if h == -128:
            continue
        count = h + 1 if h >= 0 else 1 - h
        if count > need - len(out):
            return OVERRUN, bytes(out)
        if h >= 0:
            if count > len(body) - at:
                return SHORT, bytes(out)
            out += body[at:at + count]
            at += count
        else:
            if at >= len(body):
                return SHORT, bytes(out)
            out += body[at:at + 1] * count
            at += 1
    return 0, bytes(out)


def copy_decode(body, need):
    if len(body) < need:
        return SHORT, b""
    return 0, bytes(body[:need])


def decode_strip(body, need, compression):
    if compression == LZW:
        return lzw_decode(body, need)
    if compression == PACKBITS:
        return packbits_decode(body, need)
    return copy_decode(body, need)


def finish(raw, height, width, channels, predictor, photometric):
    """u8 [H, W(, 3)] from the decoded bytes of a frame (u8 [H * W * channels])."""
    a = np.asarray(raw, np.uint8).reshape(height, width, channels)
    if predictor == 2:
        a = np.cumsum(a, axis=1, dtype=np.uint32).astype(np.uint8)
    if photometric == 0:
        a = ~a
    if channels == 3:
        a = a[:, :, ::-1]
    return np.ascontiguousarray(a.reshape((height, width) if channels == 1 else (height, width, 3)))


def decode_frame(bodies, rows_per_strip, height, width, channels, compression, predictor, photometric):
    """(status, frame or None) of one frame given the bodies of its strips in order.  A flagged frame's pixels are undefined."""
    row_bytes = width * channels
    raw = bytearray()
    status = 0
    for k, body in enumerate(bodies):
        rows = min(rows_per_strip, height - k * rows_per_strip)
        st, data = decode_strip(body, rows * row_bytes, compression)
        status |= st
        raw += data.ljust(rows * row_bytes, b"\0")
    if status:
        return status, None
    return 0, finish(np.frombuffer(bytes(raw), np.uint8), height, width, channels, predictor, photometric)


# ---- encoders for hand-built streams ------------------------------------------------------------------------------------------------
def pack_codes(codes_and_widths):
    """MSB-first bit string of (code, width) pairs, padded with zero bits to a whole byte."""
    acc = nbits = 0
    for code, width in codes_and_widths:
        acc = (acc << width) | code
        nbits += width
    pad = -nbits % 8
    return (acc << pad).to_bytes((nbits + pad) // 8, "big")


def lzw_literals(data, clear=True, eoi=True):
    """``data`` as one literal code per byte (fewer than 253 bytes: the width stays 9)."""
    assert len(data) < 253
    return pack_codes(([(CLEAR, 9)] if clear else []) + [(b, 9) for b in bytes(data)] + ([(EOI, 9)] if eoi else []))


def _width(n):
    """Bits of the next code after ``n`` data codes since the Clear: the decoder's next free entry is 257 + n."""
    free = FIRST - 1 + n
    return 9 if n == 0 else 12 if free >= 2047 else 11 if free >= 1023 else 10 if free >= 511 else 9


def lzw_encode(data, clear_after=MAX_RUN - 2):
    """A TIFF 6.0 LZW stream of ``data``: leading Clear, a Clear after ``clear_after`` data codes (libtiff's encoder clears when
    its next entry would be 4094), EOI.  Greedy longest match, as every encoder's."""
    data = bytes(data)
    out, table, n, w = [(CLEAR, 9)], {}, 0, b""

    def emit(string):
        nonlocal n, table
        out.append((string[0] if len(string) == 1 else table[string], _width(n)))
        n += 1
        if n >= clear_after:
            out.append((CLEAR, _width(n)))
            n, table = 0, {}
            return True
        return False

    for k in range(len(data)):
        wc = w + data[k:k + 1]
        if len(wc) == 1 or wc in table:
            w = wc
            continue
        entry = FIRST + n                       # the entry this code and the next byte make: 257 + (n + 1)
        if not emit(w):
            table[wc] = entry
        w = data[k:k + 1]
    if w:
        emit(w)
    out.append((EOI, _width(n)))
    return pack_codes(out)
