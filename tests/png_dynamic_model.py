"""NumPy / Python restatement of ``ysmr_png_deflate_dynamic`` and ``ysmr_png_code_lengths`` (csrc/png.hip,
csrc/png_codes.h, include/ysmr_hip.h).

The zlib stream of a canvas' PNG scanlines: 78 01, ONE deflate block with BFINAL = 1 and BTYPE = 10 (RFC 1951, 3.2.7), the
end-of-block code, padding to a byte, Adler-32 big-endian.  Scanlines, pieces, checksum and bit packing are
``png_deflate_model``'s.

Parse: a piece is parsed on its own, greedily, with the four distances 3, S, S - 3, S + 3.  A distance d is eligible at
stream position p when d <= 32768 and p >= d (``raw[d:] == raw[:-d]`` is the definition of a match's bytes).  At a byte the
longest eligible match wins, every length capped at 258 and at the piece's end; it needs 3 bytes at distance 3 and 4 at the
others; ties go in the order 3, S, S - 3, S + 3; otherwise the byte is a literal.

Code lengths (``code_lengths``), for counts[0..n) and a limit ``max_bits``:
  1. the used symbols (count > 0) ascending by (count, symbol);
  2. none used: all lengths 0; one used: length 1;
  3. Huffman's tree with two queues -- the sorted leaves, and the internal nodes in the order they were made; the lighter
     head is taken, the leaf on a tie;
  4. a leaf deeper than max_bits counts as one of depth max_bits; while the Kraft sum in units of 2^-max_bits exceeds
     2^max_bits: one code of max_bits bits less, one code less at the longest length i < max_bits that has one, two more at
     i + 1;
  5. the lengths go, shortest first, to the symbols in descending (count, symbol).
Codes are canonical (RFC 1951, 3.2.2).  The distance histogram always has two used symbols: while it has fewer, the lowest
unused symbol counts once.  Header: HLIT, HDIST, HCLEN without trailing zero lengths; the two length sequences are run-length
coded as one sequence, run by run of equal values -- r zeros: 18 (up to 138) while r >= 11, then 17 if r >= 3, then single
zeros; r lengths v > 0: v, then 16 (up to 6) while r >= 3 remain, then single v's."""
import functools
import heapq
import zlib

import numpy as np

import png_deflate_model as pm

N_LITLEN, N_DIST, N_CLEN = 286, 30, 19
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS_MAX = 3 + 5 + 5 + 4 + 3 * N_CLEN + (N_LITLEN + N_DIST) * 14
MIN_LENGTH = (3, 4, 4, 4)

_LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227]


def distances(w):
    """The four distances in tie order."""
    s = 1 + 3 * w
    return (3, s, s - 3, s + 3)


def tokens(rgb, use=(0, 1, 2, 3)):
    """The parse: ('lit', byte) and ('match', length, distance), and the stream position of every token.  ``use``: which of
    the four distances are searched."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    raw = pm.scanlines(rgb)
    n = len(raw)
    dist = distances(w)
    runs = []
    for k in range(4):
        d = dist[k]
        eq = np.zeros(n, bool)
        if k in use and d <= 32768 and d < n:
            eq[d:] = raw[d:] == raw[:-d]
        runs.append(pm._runs(eq).tolist())
    data = raw.tolist()
    out, where = [], []
    for start, length in pm.pieces(w, h):
        i, end = start, start + length
        while i < end:
            cap = min(pm.MAX_MATCH, end - i)
            best, which = 0, 0
            for k in range(4):
                l = min(runs[k][i], cap)
                if l >= MIN_LENGTH[k] and l > best:
                    best, which = l, k
            where.append(i)
            if best:
                out.append(("match", best, dist[which]))
                i += best
            else:
                out.append(("lit", data[i]))
                i += 1
    return out, where


def length_symbol(length):
    """(symbol, extra bits, their value)"""
    if length == 258:
        return 285, 0, 0
    k = max(j for j in range(28) if _LENGTH_BASE[j] <= length)
    return 257 + k, (0 if k < 8 else (k - 4) // 4), length - _LENGTH_BASE[k]


def distance_symbol(dist):
    code, base, extra_bits = 0, 1, 0
    for c in range(30):
        eb = 0 if c < 4 else c // 2 - 1
        first = 1 + c if c < 4 else 1 + ((2 + (c & 1)) << eb)
        if first <= dist:
            code, base, extra_bits = c, first, eb
    return code, extra_bits, dist - base


def histograms(toks):
    """(286 literal/length counts with the end of block, 30 distance counts with the two-code rule applied)"""
    lit, dist = [0] * N_LITLEN, [0] * N_DIST
    for tok in toks:
        if tok[0] == "lit":
            lit[tok[1]] += 1
        else:
            lit[length_symbol(tok[1])[0]] += 1
            dist[distance_symbol(tok[2])[0]] += 1
    lit[256] += 1
    return lit, force_two(dist)


def force_two(counts):
    counts = list(counts)
    for s in range(len(counts)):
        if sum(c != 0 for c in counts) >= 2:
            break
        if not counts[s]:
            counts[s] = 1
    return counts


def huffman_depths(weights):
    """Depths of the leaves of Huffman's tree over ``weights`` (sorted ascending), two queues, the leaf on a tie."""
    m = len(weights)
    weight = list(weights) + [0] * (m - 1)
    link = [0] * (2 * m - 1)
    leaf, node = 0, m
    for made in range(m, 2 * m - 1):
        total = 0
        for _ in range(2):
            if leaf < m and (node >= made or weight[leaf] <= weight[node]):
                at, leaf = leaf, leaf + 1
            else:
                at, node = node, node + 1
            total += weight[at]
            link[at] = made
        weight[made] = total
    link[2 * m - 2] = 0
    for k in range(2 * m - 3, -1, -1):
        link[k] = link[link[k]] + 1
    return link[:m]


def code_lengths(counts, max_bits):
    counts = [int(c) for c in counts]
    n = len(counts)
    order = sorted((s for s in range(n) if counts[s]), key=lambda s: (counts[s], s))
    m = len(order)
    lengths = [0] * n
    if m == 0:
        return lengths
    if m == 1:
        lengths[order[0]] = 1
        return lengths
    assert m <= 1 << max_bits
    num = [0] * (max_bits + 1)
    for d in huffman_depths([counts[s] for s in order]):
        num[min(d, max_bits)] += 1
    total = sum(num[i] << (max_bits - i) for i in range(1, max_bits + 1))
    rounds = 0
    while total > 1 << max_bits:
        assert rounds < m
        rounds += 1
        i = max(k for k in range(1, max_bits) if num[k])
        num[max_bits] -= 1
        num[i] -= 1
        num[i + 1] += 2
        total -= 1
    j = m
    for length in range(1, max_bits + 1):
        for _ in range(num[length]):
            j -= 1
            lengths[order[j]] = length
    return lengths


def optimal_cost_and_depth(counts):
    """(sum of count * length, largest length) of an unrestricted Huffman code, by a heap: no tie rule changes the total."""
    heap = [(int(c), 0) for c in counts if c]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def canonical(lengths):
    """[(code reversed for the packer, length)] per symbol (RFC 1951, 3.2.2)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if l:
            out.append((pm._reverse(nxt[l], l), l))
            nxt[l] += 1
        else:
            out.append((0, 0))
    return out


def header(lit_lengths, dist_lengths):
    """(values, bit counts) of the block's header, BFINAL and BTYPE included."""
    n_lit, n_dist = N_LITLEN, N_DIST
    while n_lit > 257 and not lit_lengths[n_lit - 1]:
        n_lit -= 1
    while n_dist > 1 and not dist_lengths[n_dist - 1]:
        n_dist -= 1
    seq = list(lit_lengths[:n_lit]) + list(dist_lengths[:n_dist])
    toks = []                                                   # (symbol, extra bits, their value)
    i = 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                toks.append((18, 7, k - 11))
                r -= k
            if r >= 3:
                toks.append((17, 3, r - 3))
                r = 0
        else:
            toks.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                toks.append((16, 2, k - 3))
                r -= k
        toks.extend([(v, 0, 0)] * r)
    cl_counts = [0] * N_CLEN
    for sym, _, _ in toks:
        cl_counts[sym] += 1
    cl_lengths = code_lengths(cl_counts, 7)
    cl_codes = canonical(cl_lengths)
    n_cl = N_CLEN
    while n_cl > 4 and not cl_lengths[CL_ORDER[n_cl - 1]]:
        n_cl -= 1
    values, counts = [0b101, n_lit - 257, n_dist - 1, n_cl - 4], [3, 5, 5, 4]      # BFINAL = 1, BTYPE = 10 with its low bit first
    for k in range(n_cl):
        values.append(cl_lengths[CL_ORDER[k]]), counts.append(3)
    for sym, extra_bits, extra in toks:
        values.append(cl_codes[sym][0]), counts.append(cl_codes[sym][1])
        if extra_bits:
            values.append(extra), counts.append(extra_bits)
    return values, counts


def deflate(rgb):
    """The stream's bytes."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    toks, _ = tokens(rgb)
    lit_counts, dist_counts = histograms(toks)
    lit_lengths, dist_lengths = code_lengths(lit_counts, 15), code_lengths(dist_counts, 15)
    lit_codes, dist_codes = canonical(lit_lengths), canonical(dist_lengths)
    values, counts = header(lit_lengths, dist_lengths)
    assert sum(counts) <= HEADER_BITS_MAX

    @functools.lru_cache(None)
    def length_bits(length):
        sym, eb, e = length_symbol(length)
        code, bits = lit_codes[sym]
        return code | e << bits, bits + eb

    @functools.lru_cache(None)
    def distance_bits(dist):
        sym, eb, e = distance_symbol(dist)
        code, bits = dist_codes[sym]
        return code | e << bits, bits + eb

    for tok in toks:
        if tok[0] == "lit":
            values.append(lit_codes[tok[1]][0]), counts.append(lit_codes[tok[1]][1])
        else:
            v, c = length_bits(tok[1])
            values.append(v), counts.append(c)
            v, c = distance_bits(tok[2])
            values.append(v), counts.append(c)
    values.append(lit_codes[256][0]), counts.append(lit_codes[256][1])
    return b"\x78\x01" + pm._pack(values, counts) + pm.adler32(pm.scanlines(rgb), w, h).to_bytes(4, "big")


def stream_bytes_bound(w, h):
    """The documented bound, before rounding to a word: the longest header, 15 bits a byte, the end of block."""
    return (HEADER_BITS_MAX + 15 * h * (1 + 3 * w) + 15 + 7) // 8 + 6


# ---- the inputs ------------------------------------------------------------------------------------------------------

def _random(w, h, rng):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _diagonal(step):
    """Every row is the row above shifted by one pixel (``step`` = 1: to the right, so the pixel above-left repeats and the
    distance is S + 3; -1: to the left, S - 3), with a few random pixels mixed in."""
    def make(w, h, rng):
        rgb = np.zeros((h, w, 3), np.uint8)
        rgb[0] = rng.integers(0, 256, (w, 3), dtype=np.uint8)
        for r in range(1, h):
            rgb[r] = np.roll(rgb[r - 1], step, axis=0)
            rgb[r, 0 if step > 0 else w - 1] = rng.integers(0, 256, 3, dtype=np.uint8)
            for x in rng.integers(0, w, 1 + w // 97):
                rgb[r, x] = rng.integers(0, 256, 3, dtype=np.uint8)
        return rgb
    return make


def _doubling(k):
    """Byte values with the counts 1, 1, 2, 4, ..., 2^k, shuffled: Huffman's tree over them is a chain."""
    def make(w, h, rng):
        n = 3 * w * h
        flat = np.full(n, k + 2, np.uint8)                      # what the doublings leave over is one more value
        reps = [1] + [1 << j for j in range(k + 1)]
        assert sum(reps) <= n
        flat[:sum(reps)] = np.repeat(np.arange(len(reps), dtype=np.uint8), reps)
        return rng.permutation(flat).reshape(h, w, 3)
    return make


def _distance_one(w, h, rng):
    """W = 1: a row of zeros under a row that ends in a zero -- four bytes repeat the byte before them, and no other
    distance has them."""
    assert w == 1
    rgb = np.zeros((h, 1, 3), np.uint8)
    rgb[0, 0] = (7, 9, 0)
    return rgb


LIMITER_CASE = "doubling-700x125"


def case_list():
    out = []
    for w in (1, 2):
        for h in (1, 2, 3):
            out.append(("white", pm._white, w, h))
            out.append(("random", _random, w, h))
            out.append(("repeat_rows", pm._repeat_rows, w, h))
    out.append(("distance_one", _distance_one, 1, 2))
    out.append(("distance_one", _distance_one, 1, 3))
    for w in (342, 700):
        out.append(("diagonal_left", _diagonal(-1), w, 67))
        out.append(("diagonal_right", _diagonal(1), w, 67))
    out.append(("doubling", _doubling(17), 700, 125))
    return [("{}-{}x{}".format(name, w, h), make, w, h) for name, make, w, h in out]


_OWN = case_list()
CASES = list(pm.CASES) + [c for c in _OWN if c[0] not in pm.CASE_IDS]
CASE_IDS = [c[0] for c in CASES]
RANDOM_LITERAL_IDS = [i for i in CASE_IDS if i.startswith("random")]


@functools.lru_cache(None)
def canvas(case_id):
    name, make, w, h = CASES[CASE_IDS.index(case_id)]
    if case_id in pm.CASE_IDS:
        return pm.case(case_id)[0]
    rgb = make(w, h, np.random.default_rng(zlib.crc32(case_id.encode())))
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(None)
def case(case_id):
    """(rgb, the model's stream) of a case; computed once, shared by the tests, not to be written to."""
    rgb = canvas(case_id)
    return rgb, deflate(rgb)


def track_canvas(w=1754, h=1240, n_tracks=125, n_steps=300, seed=11):
    """Random-walk tracks of plus-shaped dots on white with grey grid lines."""
    rng = np.random.default_rng(seed)
    rgb = np.full((h, w, 3), 255, np.uint8)
    rgb[::124, :] = 176
    rgb[:, ::175] = 176
    for _ in range(n_tracks):
        colour = rng.integers(0, 256, 3, dtype=np.uint8)
        x, y = float(rng.integers(0, w)), float(rng.integers(0, h))
        heading = rng.uniform(0, 2 * np.pi)
        for _ in range(n_steps):
            heading += rng.normal(0, 0.3)
            x, y = x + 1.5 * np.cos(heading), y + 1.5 * np.sin(heading)
            xi, yi = int(round(x)), int(round(y))
            if 1 <= xi < w - 1 and 1 <= yi < h - 1:
                rgb[yi, xi - 1:xi + 2] = colour
                rgb[yi - 1:yi + 2, xi] = colour
    return rgb
