"""The figures' PNG files on the device, the parts that need no GPU: the model of the deflate stream (tests/png_deflate_model.py)
against zlib, the recorded lettering against the host's stamping, the C ABI's declarations and argument checks."""
import os
import re
import zlib

import numpy as np
import pytest

import png_deflate_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ysmr_png_workspace_bytes", "ysmr_png_stream_bytes_max", "ysmr_png_deflate", "ysmr_plot_stamp")


# ---- the model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", pm.CASE_IDS)
def test_model_stream_decompresses_to_the_scanlines(case_id):
    rgb, stream = pm.case(case_id)
    raw = pm.scanlines(rgb).tobytes()
    assert stream[:2] == b"\x78\x01" and stream[2] & 7 == 0b011               # one final block in the fixed code
    assert zlib.decompress(stream) == raw
    assert len(stream) <= pm.stream_bytes_bound(rgb.shape[1], rgb.shape[0])
    d = zlib.decompressobj()
    assert d.decompress(stream) == raw and d.eof and d.unused_data == b""     # nothing behind the checksum


@pytest.mark.parametrize("case_id", pm.CASE_IDS)
def test_model_adler_is_zlibs(case_id):
    rgb, stream = pm.case(case_id)
    raw = pm.scanlines(rgb)
    want = zlib.adler32(raw.tobytes()) & 0xFFFFFFFF
    assert pm.adler32(raw, rgb.shape[1], rgb.shape[0]) == want
    assert int.from_bytes(stream[-4:], "big") == want


def test_model_parse_keeps_the_rules():
    """No match crosses a piece's end or is longer than 258; the row distance appears iff S <= 32768; matches have the
    minimum lengths 3 (distance 3) and 4 (distance S)."""
    seen = set()
    for case_id in ("piece_ends-700x2", "runs_600_271-700x67", "runs_1_370-342x67", "repeat_rows-10922x3", "repeat_rows-10923x3",
                    "periods-341x67"):
        rgb, _ = pm.case(case_id)
        h, w = rgb.shape[:2]
        s = 1 + 3 * w
        ends = {start + length for start, length in pm.pieces(w, h)}
        at = 0
        for tok in pm.tokens(rgb):
            n = 1 if tok[0] == "lit" else tok[1]
            if tok[0] == "match":
                assert 3 <= n <= 258 and tok[2] in (3, s) and (tok[2] == 3 or (n >= 4 and s <= 32768))
                assert at - tok[2] >= 0
                seen.add((case_id, "row" if tok[2] == s else "pixel"))
                if n == 258:
                    seen.add("cap")
            nxt = min(e for e in ends if e > at)
            assert at + n <= nxt, "a token crosses the piece's end at {}".format(nxt)
            if tok[0] == "match" and at + n == nxt:
                seen.add((case_id, "ends at a piece's end"))
            at += n
        assert at == h * s
    assert ("repeat_rows-10922x3", "row") in seen and ("repeat_rows-10923x3", "row") not in seen
    assert ("piece_ends-700x2", "ends at a piece's end") in seen and "cap" in seen


def test_random_literals_come_close_to_the_bound():
    rgb, stream = pm.case("random144-341x67")
    bound = pm.stream_bytes_bound(341, 67)
    assert 0.98 * bound <= len(stream) <= bound


# ---- the lettering ---------------------------------------------------------------------------------------------------

def _replay(shape, decorate):
    from ysmr_amd import plot_functions as pf
    want = np.full(shape, 255, np.uint8)
    decorate(want)
    stamps = pf.StampList(shape[0], shape[1])
    decorate(stamps)
    records, bits = stamps.arrays()
    got = pm.paint_stamps(np.full(shape, 255, np.uint8), records, bits)
    assert len(records) > 5 and (want != 255).any()
    assert np.array_equal(got, want), "{} pixels differ".format((got != want).any(axis=2).sum())
    return records


@pytest.mark.parametrize("size,dpi", [((1169, 826), 100), ((300, 200), 300), ((3507, 2480), 300)])
def test_recorded_track_lettering_replays_to_the_hosts_canvas(size, dpi):
    from ysmr_amd import plot_functions as pf
    view, cols, rows = pf.track_view((-12.5, 310.0, 3.0, 190.25), 0, 1.7, dpi, size=size)
    _replay((size[1], size[0], 3), lambda canvas: pf.decorate_track_figure(canvas, view, cols, rows, "12. 03. '21, clip µ", 0.5, 212.125, dpi))


@pytest.mark.parametrize("size,dpi", [((1753, 1240), 300), ((240, 150), 300)])
def test_recorded_violin_lettering_replays_to_the_hosts_canvas(size, dpi):
    from ysmr_amd import _lib
    from ysmr_amd import plot_functions as pf
    sums = np.zeros(4, _lib.VIOLIN_SUMMARY_DTYPE)
    sums["members"], sums["values"] = [40, 25, 0, 15], [40, 25, 0, 15]
    sums["vmin"], sums["vmax"], sums["q50"], sums["mean"] = 1.0, 9.5, 4.25, 4.5
    labels = ["All", "Immotile", "Between", "Motile"]
    view, rows = pf.violin_view(sums, None, None, dpi, size=size)
    boxes = pf.violin_text_boxes(sums, labels)
    records = _replay((size[1], size[0], 3),
                      lambda canvas: pf.decorate_violin_figure(canvas, view, rows, "clip", "Speed (µm/s)", labels, boxes, dpi))
    assert (records["h"] > records["w"]).any()                               # the column's name, reading upwards


def test_recorded_angle_lettering_replays_to_the_hosts_canvas():
    from ysmr_amd import plot_functions as pf
    W, H = 1169, 826
    cx, cy, ring_r2, _ = pf.wedge_plan([3, 9, 4], W, H)
    _replay((H, W, 3), lambda canvas: pf.decorate_angle_figure(canvas, W, H, cx, cy, ring_r2, "clip", 4711, 9, 100))


def test_stamp_functions_keep_their_behaviour_on_a_canvas():
    from ysmr_amd import plot_functions as pf
    rgb = np.full((30, 40, 3), 255, np.uint8)
    pf.stamp_text(rgb, -3, 25, "Ag", 2, colour=(1, 2, 3))                     # clipped left and below
    bm = pf.text_bitmap("Ag", 2)
    want = np.full((30, 40, 3), 255, np.uint8)
    want[25:30, 0:bm.shape[1] - 3][bm[:5, 3:]] = (1, 2, 3)
    assert np.array_equal(rgb, want)
    pf.stamp_text_vertical(rgb, 38, 1, "b", 1)                                # clipped above and on the right
    v = np.rot90(pf.text_bitmap("b", 1))
    y = 1 - v.shape[0] // 2
    want[0:y + v.shape[0], 38:40][v[-y:, :2]] = (0, 0, 0)
    assert np.array_equal(rgb, want)


# ---- the C ABI -------------------------------------------------------------------------------------------------------

def test_header_declares_the_new_exports_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", text), name
    assert re.search(r"#define\s+YSMR_ABI_VERSION\s+15\b", text)
    assert "typedef struct ysmr_stamp" in text


def test_library_exports_and_binding():
    from ysmr_amd import _lib
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.STAMP_DTYPE.itemsize == 24 and L.ysmr_abi_version() == 15


def test_sizes_and_argument_checks_on_the_host():
    from ysmr_amd import _lib
    L = _lib.lib()
    for w, h in pm.SHAPES + [(3507, 2480), (16384, 16384)]:
        assert L.ysmr_png_stream_bytes_max(w, h) >= pm.stream_bytes_bound(w, h)
        assert L.ysmr_png_stream_bytes_max(w, h) <= pm.stream_bytes_bound(w, h) + 8
        assert L.ysmr_png_workspace_bytes(w, h) > 0
    for w, h in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5)):
        assert L.ysmr_png_workspace_bytes(w, h) == 0 and L.ysmr_png_stream_bytes_max(w, h) == 0
        assert L.ysmr_png_deflate(None, 4096, w, h, 4096, 1 << 30, 4096, 1 << 30, 4096) == _lib.YSMR_ERR_ARG
        assert b"16384" in L.ysmr_last_error()
    ws, out = L.ysmr_png_workspace_bytes(85, 2), L.ysmr_png_stream_bytes_max(85, 2)
    # (the pointers are never followed: every check comes before the first launch)
    assert L.ysmr_png_deflate(None, 4096, 85, 2, 4096, ws - 1, 4096, out, 4096) == _lib.YSMR_ERR_ARG
    assert b"workspace" in L.ysmr_last_error()
    assert L.ysmr_png_deflate(None, 4096, 85, 2, 4096, ws, 4096, out - 1, 4096) == _lib.YSMR_ERR_ARG
    assert b"output" in L.ysmr_last_error()
    assert L.ysmr_png_deflate(None, None, 85, 2, 4096, ws, 4096, out, 4096) == _lib.YSMR_ERR_ARG
    assert L.ysmr_plot_stamp(None, 4096, 0, 5, 4096, 1, 4096, 8) == _lib.YSMR_ERR_ARG
    assert L.ysmr_plot_stamp(None, 4096, 5, 5, 4096, -1, 4096, 8) == _lib.YSMR_ERR_ARG
    assert L.ysmr_plot_stamp(None, 4096, 5, 5, 4096, 4097, 4096, 8) == _lib.YSMR_ERR_ARG
    assert L.ysmr_plot_stamp(None, None, 5, 5, 4096, 1, 4096, 8) == _lib.YSMR_ERR_ARG
    assert L.ysmr_plot_stamp(None, 4096, 5, 5, 4096, 0, 4096, 8) == _lib.YSMR_OK      # nothing to paint, nothing launched


def test_figure_functions_take_the_keyword():
    import inspect
    from ysmr_amd import plot_functions as pf
    for f in (pf.large_xy_plot, pf.rose_graph, pf.angle_distribution_plot, pf.violin_plot):
        assert inspect.signature(f).parameters["png_on_device"].default is False
    assert callable(pf.write_png_device) and callable(pf.write_png) and callable(pf.stamp_text_vertical)
