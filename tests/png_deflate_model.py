"""NumPy / Python restatement of ``ysmr_png_deflate`` (csrc/png.hip, include/ysmr_hip.h) and of ``ysmr_plot_stamp``.

The zlib stream of a canvas' PNG scanlines: 78 01, one deflate block in the fixed Huffman code (RFC 1951, 3.2.6), the
end-of-block code, padding to a byte, Adler-32 big-endian.  The scanline stream is H rows of S = 1 + 3 W bytes (a filter
byte 0 in front of every row); every row is cut into pieces of 1024 bytes, the last one shorter, and a piece is parsed on
its own, greedily, with the two distances 3 and S (S only while S <= 32768): no match extends past its piece's end, its
source may lie anywhere earlier in the stream.  Huffman codes go into the stream most significant bit first, extra bits
least significant bit first, bytes are filled from bit 0.

Also here: the inputs the CPU and the GPU tests share (``cases``), and a painter that replays a recorded stamp list."""
import functools
import zlib

import numpy as np

PIECE = 1024
MAX_MATCH = 258
ADLER = 65521


def scanlines(rgb):
    """u8 [H * (1 + 3 W)]: the bytes a PNG of filter 0 deflates."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = rgb.reshape(h, 3 * w)
    return raw.reshape(-1)


def pieces(w, h):
    """(start, length) of every piece in stream order."""
    s = 1 + 3 * w
    return [(r * s + c, min(PIECE, s - c)) for r in range(h) for c in range(0, s, PIECE)]


def adler32(raw, w, h):
    """Per-piece sums (a2, b2 of the piece alone, starting from 0) combined in order: a = a1 + a2,
    b = b1 + b2 + len2 * a1 -- the standard rule, b1 + b2' + len2 (a1 - 1) for checksums that each start at a = 1."""
    a, b = 1, 0
    for start, length in pieces(w, h):
        part = raw[start:start + length].astype(np.uint64)
        a2 = int(part.sum()) % ADLER
        b2 = int((part * np.arange(length, 0, -1, dtype=np.uint64)).sum()) % ADLER
        b = (b + b2 + length * a) % ADLER
        a = (a + a2) % ADLER
    return b << 16 | a


def _runs(eq):
    """run[i]: the number of consecutive true entries of ``eq`` from i on."""
    n = len(eq)
    stop = np.where(eq, n, np.arange(n))                      # a false entry stops a run at itself
    nxt = np.minimum.accumulate(stop[::-1])[::-1]
    return nxt - np.arange(n)


def _reverse(code, bits):
    return int("{:0{}b}".format(code, bits)[::-1], 2)


def _literal(v):
    return (_reverse(0x30 + v, 8), 8) if v < 144 else (_reverse(0x190 + v - 144, 9), 9)


def _length(length):
    """(bits as they enter the stream, their number): the symbol's Huffman code, then its extra bits."""
    if length == 258:
        sym, extra_bits, extra = 285, 0, 0
    else:
        base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227]
        k = max(j for j in range(28) if base[j] <= length)
        sym, extra_bits, extra = 257 + k, (0 if k < 8 else (k - 4) // 4), length - base[k]
    code, bits = (sym - 256, 7) if sym < 280 else (0xC0 + sym - 280, 8)
    return _reverse(code, bits) | extra << bits, bits + extra_bits


def _distance(dist):
    """5 code bits, most significant first, then the extra bits (RFC 1951, 3.2.5)."""
    code, base, extra_bits = 0, 1, 0
    for c in range(30):
        eb = 0 if c < 4 else c // 2 - 1
        first = 1 + c if c < 4 else 1 + ((2 + (c & 1)) << eb)
        if first <= dist:
            code, base, extra_bits = c, first, eb
    return _reverse(code, 5) | (dist - base) << 5, 5 + extra_bits


def tokens(rgb):
    """The parse: a list of ('lit', byte) and ('match', length, distance)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    s = 1 + 3 * w
    raw = scanlines(rgb)
    n = len(raw)
    eq3, eqs = np.zeros(n, bool), np.zeros(n, bool)
    eq3[3:] = raw[3:] == raw[:-3]
    if s <= 32768:
        eqs[s:] = raw[s:] == raw[:-s]
    run3, runs = _runs(eq3).tolist(), _runs(eqs).tolist()
    data = raw.tolist()
    out = []
    for start, length in pieces(w, h):
        i, end = start, start + length
        while i < end:
            cap = min(MAX_MATCH, end - i)
            l3, ls = min(run3[i], cap), min(runs[i], cap)
            if l3 >= ls and l3 >= 3:
                out.append(("match", l3, 3))
                i += l3
            elif ls >= 4:
                out.append(("match", ls, s))
                i += ls
            elif l3 >= 3:
                out.append(("match", l3, 3))
                i += l3
            else:
                out.append(("lit", data[i]))
                i += 1
    return out


def _pack(values, counts):
    """Bit strings (value, number of bits <= 31), each least significant bit first, one after the other; bytes fill from bit 0."""
    values, counts = np.asarray(values, np.int64), np.asarray(counts, np.int64)
    at = np.concatenate([[0], np.cumsum(counts)])
    bits = np.zeros(int(at[-1]) + (-int(at[-1])) % 8, np.uint8)
    for k in range(int(counts.max())):
        on = counts > k
        bits[at[:-1][on] + k] = (values[on] >> k) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def deflate(rgb):
    """The stream's bytes."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    values, counts = [0b011], [3]                               # BFINAL = 1, then BTYPE = 01 with its low bit first
    length_of, dist_of = functools.lru_cache(None)(_length), functools.lru_cache(None)(_distance)
    for tok in tokens(rgb):
        if tok[0] == "lit":
            v, c = _literal(tok[1])
            values.append(v), counts.append(c)
        else:
            v, c = length_of(tok[1])
            values.append(v), counts.append(c)
            v, c = dist_of(tok[2])
            values.append(v), counts.append(c)
    values.append(0), counts.append(7)                          # end of block: symbol 256
    return b"\x78\x01" + _pack(values, counts) + adler32(scanlines(rgb), w, h).to_bytes(4, "big")


def stream_bytes_bound(w, h):
    """The issue's bound: no code spends more than 9 bits on a byte."""
    return (3 + 9 * h * (1 + 3 * w) + 7 + 7) // 8 + 6


# ---- the inputs ------------------------------------------------------------------------------------------------------

SHAPES = [(w, h) for w in (1, 85, 341, 342, 700) for h in (1, 2, 67)] + [(10922, 3), (10923, 3)]
# strides 4, 256, 1024 (exactly one piece), 1027 (a piece and 3 bytes), 2101 (three pieces); 32767 (the row distance is
# allowed) and 32770 (it is dropped)


def _white(w, h, rng):
    return np.full((h, w, 3), 255, np.uint8)


def _random144(w, h, rng):
    return rng.integers(144, 256, (h, w, 3), dtype=np.uint8)            # 9-bit literals only, or nearly


def _runs_of(lengths):
    def make(w, h, rng):
        flat = np.zeros(3 * w * h, np.uint8)
        at, k = 0, 0
        while at < len(flat):
            n = lengths[k % len(lengths)]
            flat[at:at + n] = (37 * k + 11) % 251                        # neighbours differ
            at += n
            k += 1
        return flat.reshape(h, w, 3)
    return make


def _repeat_rows(w, h, rng):
    """Every row repeats the one above except for single pixels."""
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[0] = rng.integers(0, 256, (w, 3), dtype=np.uint8)
    for r in range(1, h):
        rgb[r] = rgb[r - 1]
        for x in rng.integers(0, w, 1 + w // 97):
            rgb[r, x] = rng.integers(0, 256, 3, dtype=np.uint8)
    return rgb


def _periods(w, h, rng):
    """Stretches of one byte value (period 1) against stretches of one colour with three different bytes (period 3),
    cut at random places; every other row repeats its predecessor in part."""
    rgb = np.zeros((h, w, 3), np.uint8)
    for r in range(h):
        x = 0
        while x < w:
            n = int(rng.integers(1, 120))
            rgb[r, x:x + n] = int(rng.integers(0, 256)) if rng.integers(0, 2) else rng.permutation(256)[:3].astype(np.uint8)
            x += n
        if r % 2 and w > 1:
            cut = int(rng.integers(0, w))
            rgb[r, cut:] = rgb[r - 1, cut:]
    return rgb


def _piece_ends(w, h, rng):
    """W = 700, S = 2101, pieces end at scanline bytes 1024 and 2048: one colour over the bytes [901, 1024) -- the match
    ends exactly at the piece's end, other bytes follow -- and over [1900, 2101), which a match would cross 2048 with; the
    rest random.  The second row (if any) repeats the first: the row distance meets the same ends."""
    assert w == 700
    row = rng.integers(0, 256, 3 * w, dtype=np.uint8)                    # row[c - 1] is scanline byte c
    row[900:1023] = np.tile(np.array([10, 200, 90], np.uint8), 41)
    row[1023] = row[1020] ^ 0x55
    row[1899:2100] = np.tile(np.array([7, 7, 250], np.uint8), 67)
    rgb = np.tile(row.reshape(1, w, 3), (h, 1, 1))
    if h > 2:
        rgb[2:] = rng.integers(0, 256, (h - 2, w, 3), dtype=np.uint8)
    return rgb


def case_list():
    """(id, maker, W, H) of every input, each id unique."""
    out = []
    for w, h in SHAPES:
        out.append(("white", _white, w, h))
        out.append(("repeat_rows", _repeat_rows, w, h))
        if h == 67 or w > 10000:
            out.append(("periods", _periods, w, h))
    for w, h in ((1, 1), (85, 2), (341, 67), (342, 67), (700, 2), (10922, 3), (10923, 3)):
        out.append(("random144", _random144, w, h))
    out.append(("runs_1_370", _runs_of(list(range(1, 371))), 342, 67))       # 68 635 of the 68 742 bytes
    out.append(("runs_600_271", _runs_of(list(range(600, 270, -1))), 700, 67))
    for h in (1, 2, 67):
        out.append(("piece_ends", _piece_ends, 700, h))
    return [("{}-{}x{}".format(name, w, h), make, w, h) for name, make, w, h in out]


CASES = case_list()
CASE_IDS = [c[0] for c in CASES]


@functools.lru_cache(None)
def case(case_id):
    """(rgb, the model's stream) of a case; computed once, shared by the tests, not to be written to."""
    name, make, w, h = CASES[CASE_IDS.index(case_id)]
    rgb = make(w, h, np.random.default_rng(zlib.crc32(case_id.encode())))
    rgb.setflags(write=False)
    return rgb, deflate(rgb)


def discs_canvas(w=3507, h=2480, n=3000, seed=7):
    """A full-size canvas: a few thousand discs of many colours on white, bounding-box painted."""
    rng = np.random.default_rng(seed)
    rgb = np.full((h, w, 3), 255, np.uint8)
    for cx, cy, rad in zip(rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(2, 14, n)):
        x0, x1, y0, y1 = max(cx - rad, 0), min(cx + rad + 1, w), max(cy - rad, 0), min(cy + rad + 1, h)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        rgb[y0:y1, x0:x1][(xx - cx) ** 2 + (yy - cy) ** 2 <= rad * rad] = rng.integers(0, 256, 3, dtype=np.uint8)
    return rgb


# ---- the lettering ---------------------------------------------------------------------------------------------------

def paint_stamps(rgb, records, bits):
    """``ysmr_plot_stamp`` on a NumPy canvas: the records (``_lib.STAMP_DTYPE``) in order, bit k of a record being
    (bits[(bit_offset + k) // 8] >> ((bit_offset + k) % 8)) & 1, pixels outside the canvas dropped."""
    H, W = rgb.shape[:2]
    unpacked = np.unpackbits(np.asarray(bits, np.uint8), bitorder="little").astype(bool)
    for rec in records:
        x, y, w, h, off, colour = (int(rec[k]) for k in ("x", "y", "w", "h", "bit_offset", "colour"))
        if w < 1 or h < 1 or off + w * h > len(unpacked):
            continue
        bm = unpacked[off:off + w * h].reshape(h, w)
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
        if x0 >= x1 or y0 >= y1:
            continue
        rgb[y0:y1, x0:x1][bm[y0 - y:y1 - y, x0 - x:x1 - x]] = (colour & 255, colour >> 8 & 255, colour >> 16 & 255)
    return rgb
