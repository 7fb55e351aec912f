"""ysmr_png_deflate_dynamic, the parts that need no GPU: the model of the stream (tests/png_dynamic_model.py) against zlib and
its own rules, ``ysmr_png_code_lengths`` of the built library against the model's code lengths, the C ABI's declarations,
and the sizes the dynamic stream is there for."""
import os
import re
import zlib

import numpy as np
import pytest

import png_deflate_model as pm
import png_dynamic_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ysmr_png_dynamic_workspace_bytes", "ysmr_png_dynamic_stream_bytes_max", "ysmr_png_deflate_dynamic", "ysmr_png_code_lengths")
OVER_THE_LIMIT = (dm.LIMITER_CASE,)      # the only cases whose unrestricted Huffman code is deeper than 15 bits


# ---- the stream ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", dm.CASE_IDS)
def test_model_stream_decompresses_to_the_scanlines(case_id):
    rgb, stream = dm.case(case_id)
    raw = pm.scanlines(rgb).tobytes()
    assert stream[:2] == b"\x78\x01" and stream[2] & 7 == 0b101               # one final block, BTYPE = 2
    assert zlib.decompress(stream) == raw
    assert len(stream) <= dm.stream_bytes_bound(rgb.shape[1], rgb.shape[0])
    d = zlib.decompressobj()
    assert d.decompress(stream) == raw and d.eof and d.unused_data == b""     # nothing behind the checksum
    assert int.from_bytes(stream[-4:], "big") == zlib.adler32(raw) & 0xFFFFFFFF


# ---- the parse -------------------------------------------------------------------------------------------------------

def _check_parse(case_id, seen):
    rgb = dm.canvas(case_id)
    h, w = rgb.shape[:2]
    s = 1 + 3 * w
    raw = pm.scanlines(rgb)
    dist = dm.distances(w)
    ends = sorted(start + length for start, length in pm.pieces(w, h))
    toks, where = dm.tokens(rgb)
    at, e = 0, 0
    for tok, pos in zip(toks, where):
        assert pos == at
        while ends[e] <= at:
            e += 1
        room = min(258, ends[e] - at)
        # the longest run of equal bytes at every eligible distance, from the definition raw[d:] == raw[:-d]
        runs = []
        for d in dist:
            n = 0
            if d <= 32768 and at >= d:
                while n < room and raw[at + n] == raw[at + n - d]:
                    n += 1
            runs.append(n)
        valid = [n if n >= dm.MIN_LENGTH[k] else 0 for k, n in enumerate(runs)]
        if tok[0] == "lit":
            assert not any(valid) and tok[1] == raw[at]
            at += 1
            continue
        _, n, d = tok
        k = dist.index(d)
        assert d <= 32768 and at >= d and dm.MIN_LENGTH[k] <= n <= room
        assert n == max(valid) and k == valid.index(n), "not the longest match, or not the first of equals"
        seen.add((case_id, k))
        if at + n == ends[e]:
            seen.add((case_id, k, "ends at a piece's end"))
        if valid.count(n) > 1:
            seen.add("tie")
        at += n
    assert at == h * s


def test_model_parse_keeps_the_rules():
    """Eligibility, the minimum lengths, the longest match and the tie order at every token, no token across a piece's end."""
    seen = set()
    ids = [i for i in dm.CASE_IDS if re.search(r"-[12]x[123]$", i)] + [
        "diagonal_left-342x67", "diagonal_right-342x67", "diagonal_left-700x67", "diagonal_right-700x67", "piece_ends-700x2",
        "repeat_rows-10922x3", "repeat_rows-10923x3", "periods-341x67", "white-700x1", "white-700x67"]
    for case_id in ids:
        _check_parse(case_id, seen)
    assert "tie" in seen
    # 1 x 1: no match at all; W = 1: S - 3 is distance 1
    assert not [t for t in dm.tokens(dm.canvas("random-1x1"))[0] if t[0] == "match"]
    assert ("white-1x1", 0) not in seen and ("distance_one-1x2", 2) in seen and ("distance_one-1x3", 2) in seen
    # S = 32767: S - 3 and S are searched, S + 3 is not; S = 32770: only 3 and S - 3
    assert ("repeat_rows-10922x3", 1) in seen and ("repeat_rows-10922x3", 3) not in seen
    assert ("repeat_rows-10923x3", 1) not in seen and ("repeat_rows-10923x3", 3) not in seen
    # the diagonals: both distances occur, each at a piece's end too, and they dominate
    for w in (342, 700):
        assert ("diagonal_left-{}x67".format(w), 2, "ends at a piece's end") in seen
        assert ("diagonal_right-{}x67".format(w), 3, "ends at a piece's end") in seen
    for case_id, d in (("diagonal_left-700x67", 2101 - 3), ("diagonal_right-700x67", 2101 + 3)):
        toks = dm.tokens(dm.canvas(case_id))[0]
        covered = sum(t[1] for t in toks if t[0] == "match" and t[2] == d)
        assert covered > 0.9 * 66 * 2101, "{}: distance {} covers {} bytes".format(case_id, d, covered)


@pytest.mark.parametrize("case_id", ["periods-341x67", "repeat_rows-342x67", "piece_ends-700x2", "white-1x67", "repeat_rows-10922x3",
                                     "repeat_rows-10923x3", "diagonal_left-342x67"])
def test_with_the_distances_3_and_S_the_parse_is_the_fixed_streams(case_id):
    rgb = dm.canvas(case_id)
    assert dm.tokens(rgb, use=(0, 1))[0] == pm.tokens(rgb)


# ---- the codes -------------------------------------------------------------------------------------------------------

def _kraft(lengths, max_bits):
    return sum(1 << (max_bits - l) for l in lengths if l)


@pytest.mark.parametrize("case_id", dm.CASE_IDS)
def test_code_lengths_are_a_prefix_code_and_optimal_below_the_limit(case_id):
    rgb = dm.canvas(case_id)
    lit, dist = dm.histograms(dm.tokens(rgb)[0])
    assert lit[256] == 1 and sum(c != 0 for c in dist) >= 2
    for counts in (lit, dist):
        lengths = dm.code_lengths(counts, 15)
        assert all((l > 0) == (c > 0) for l, c in zip(lengths, counts)) and max(lengths) <= 15
        assert _kraft(lengths, 15) <= 1 << 15
        cost, depth = dm.optimal_cost_and_depth(counts)
        got = sum(c * l for c, l in zip(counts, lengths))
        if counts is lit and case_id in OVER_THE_LIMIT:
            assert depth > 15, "the limiter case no longer needs the limiter: depth {}".format(depth)
            assert got > cost and max(lengths) == 15
        else:
            assert depth <= 15, "{} needs the limiter (depth {}) and is not listed".format(case_id, depth)
            assert got == cost


def test_all_white_uses_one_distance_and_gets_two_codes():
    toks = dm.tokens(dm.canvas("white-700x1"))[0]              # (a second row would repeat the first at distance S)
    assert {t[2] for t in toks if t[0] == "match"} == {3}
    _, dist = dm.histograms(toks)
    assert [s for s, c in enumerate(dist) if c] == [0, 2] and dist[0] == 1
    assert [l for l in dm.code_lengths(dist, 15) if l] == [1, 1]
    _, dist = dm.histograms(dm.tokens(dm.canvas("random-1x1"))[0])
    assert dist[:3] == [1, 1, 0] and sum(dist) == 2


def _library_lengths(counts, max_bits):
    from ysmr_amd import _lib
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.full(len(counts), 99, np.uint8)
    rc = _lib.lib().ysmr_png_code_lengths(counts.ctypes.data, len(counts), max_bits, out.ctypes.data)
    assert rc == _lib.YSMR_OK, _lib.lib().ysmr_last_error()
    return out.tolist()


def _agree(counts, max_bits):
    want = dm.code_lengths(counts, max_bits)
    assert _library_lengths(counts, max_bits) == want
    used = [l for l in want if l]
    assert max(want) <= max_bits and (len(used) < 2 or _kraft(want, max_bits) <= 1 << max_bits)
    cost, depth = dm.optimal_cost_and_depth(counts) if used else (0, 0)
    if depth <= max_bits:
        assert sum(int(c) * l for c, l in zip(counts, want)) == cost
    return depth


def test_library_code_lengths_are_the_models_on_random_histograms():
    rng = np.random.default_rng(20261019)
    for k in range(2000):
        n = int(rng.integers(1, 289))
        top = int(rng.choice([2, 16, 1 << 10, 1 << 26]))
        counts = rng.integers(1, top + 1, n).astype(np.uint32)
        if k % 2:                                               # sparse
            counts[rng.random(n) < rng.uniform(0.3, 0.98)] = 0
        _agree(counts, 15)


@pytest.mark.parametrize("max_bits", [15, 7])
def test_library_code_lengths_are_the_models_beyond_the_limit(max_bits):
    rng = np.random.default_rng(max_bits)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    deepest = 0
    for n in (max_bits, max_bits + 2, max_bits + 3, max_bits + 10, 26):
        pow2 = [1] + [1 << j for j in range(n - 1)]
        for base in (pow2, fib[:n], pow2 + pow2, fib[:n] + [3] * 30):
            base = [min(c, (1 << 32) - 1) for c in base]
            for counts in (base, base[::-1], rng.permutation(base).tolist(), [0, 0] + base + [0]):
                deepest = max(deepest, _agree(np.array(counts, np.uint32), max_bits))
    assert deepest > max_bits + 5                               # the limiter was needed, and by a margin


def test_library_code_lengths_edge_cases_and_argument_checks():
    from ysmr_amd import _lib
    L = _lib.lib()
    assert _library_lengths([0, 0, 0], 15) == [0, 0, 0]
    assert _library_lengths([7], 15) == [1]
    assert _library_lengths([0, 0, 5, 0], 15) == [0, 0, 1, 0] == dm.code_lengths([0, 0, 5, 0], 15)
    assert _library_lengths([0, 9, 0, 2], 1) == [0, 1, 0, 1]
    for n in (2, 3, 19, 30, 128, 286, 288):
        _agree(np.full(n, 1000, np.uint32), 15)
    assert _agree(np.full(128, 3, np.uint32), 7) == 7 and _library_lengths(np.full(128, 3, np.uint32), 7) == [7] * 128
    assert _agree(np.full(288, (1 << 32) - 1, np.uint32), 15) <= 9        # the weights add up in 64 bits
    counts, out = np.ones(4, np.uint32), np.zeros(288, np.uint8)
    big = np.ones(289, np.uint32)
    for args in ((None, 4, 15, out.ctypes.data), (counts.ctypes.data, 4, 15, None), (counts.ctypes.data, 0, 15, out.ctypes.data),
                 (big.ctypes.data, 289, 15, out.ctypes.data), (counts.ctypes.data, 4, 0, out.ctypes.data),
                 (counts.ctypes.data, 4, 16, out.ctypes.data), (counts.ctypes.data, 4, 1, out.ctypes.data)):   # the last: 4 symbols, 1 bit
        assert L.ysmr_png_code_lengths(*args) == _lib.YSMR_ERR_ARG
        assert L.ysmr_last_error()


# ---- the C ABI -------------------------------------------------------------------------------------------------------

def test_header_declares_the_new_exports_and_keeps_the_abi_version():
    from ysmr_amd import _lib
    text = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+YSMR_ABI_VERSION\s+15\b", text)
    assert _lib.lib().ysmr_abi_version() == 15


def test_sizes_and_argument_checks_on_the_host():
    from ysmr_amd import _lib
    L = _lib.lib()
    for w, h in pm.SHAPES + [(2, 3), (3507, 2480), (16384, 16384)]:
        assert dm.stream_bytes_bound(w, h) <= L.ysmr_png_dynamic_stream_bytes_max(w, h) <= dm.stream_bytes_bound(w, h) + 8
        assert L.ysmr_png_dynamic_workspace_bytes(w, h) > L.ysmr_png_workspace_bytes(w, h)
    for w, h in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5)):
        assert L.ysmr_png_dynamic_workspace_bytes(w, h) == 0 and L.ysmr_png_dynamic_stream_bytes_max(w, h) == 0
        assert L.ysmr_png_deflate_dynamic(None, 4096, w, h, 4096, 1 << 30, 4096, 1 << 30, 4096) == _lib.YSMR_ERR_ARG
        assert b"16384" in L.ysmr_last_error()
    ws, out = L.ysmr_png_dynamic_workspace_bytes(85, 2), L.ysmr_png_dynamic_stream_bytes_max(85, 2)
    # (the pointers are never followed: every check comes before the first launch)
    assert L.ysmr_png_deflate_dynamic(None, 4096, 85, 2, 4096, ws - 1, 4096, out, 4096) == _lib.YSMR_ERR_ARG
    assert b"workspace" in L.ysmr_last_error()
    assert L.ysmr_png_deflate_dynamic(None, 4096, 85, 2, 4096, ws, 4096, out - 1, 4096) == _lib.YSMR_ERR_ARG
    assert b"output" in L.ysmr_last_error()
    for args in ((None, 85, 2, 4096, ws, 4096, out, 4096), (4096, 85, 2, None, ws, 4096, out, 4096), (4096, 85, 2, 4096, ws, None, out, 4096),
                 (4096, 85, 2, 4096, ws, 4096, out, None), (4096, 85, 2, 4100, ws, 4096, out, 4096), (4096, 85, 2, 4096, ws, 4098, out, 4096),
                 (4096, 85, 2, 4096, ws, 4096, out, 4100)):
        assert L.ysmr_png_deflate_dynamic(None, *args) == _lib.YSMR_ERR_ARG


def test_python_surface_takes_the_keyword():
    import inspect
    from ysmr_amd import plot_functions as pf
    assert inspect.signature(pf.device_deflate).parameters["dynamic"].default is False
    assert inspect.signature(pf.write_png_device).parameters["dynamic"].default is False
    assert pf.png_mode(False) is None and pf.png_mode(None) is None and pf.png_mode(0) is None
    assert pf.png_mode(True) == "fixed" and pf.png_mode(1) == "fixed" and pf.png_mode("yes") == "fixed"
    assert pf.png_mode("dynamic") == pf.png_mode("Dynamic") == pf.png_mode(" DYNAMIC ") == "dynamic"


# ---- what it is for --------------------------------------------------------------------------------------------------

def test_dynamic_stream_is_shorter_than_the_fixed_one_on_the_discs():
    rgb = pm.discs_canvas()
    dynamic, fixed = len(dm.deflate(rgb)), len(pm.deflate(rgb))
    print("discs 3507 x 2480: dynamic {} B, fixed {} B, zlib level 1 {} B".format(dynamic, fixed, len(zlib.compress(pm.scanlines(rgb).tobytes(), 1))))
    assert dynamic < fixed


def test_dynamic_stream_on_a_track_canvas_beats_the_fixed_one_and_zlib_level_1():
    rgb = dm.track_canvas()
    raw = pm.scanlines(rgb).tobytes()
    stream = dm.deflate(rgb)
    assert zlib.decompress(stream) == raw
    dynamic, fixed, host = len(stream), len(pm.deflate(rgb)), len(zlib.compress(raw, 1))
    print("tracks 1754 x 1240: dynamic {} B, fixed {} B, zlib level 1 {} B".format(dynamic, fixed, host))
    assert dynamic < fixed
    assert dynamic <= host
