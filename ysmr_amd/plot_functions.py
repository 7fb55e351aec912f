"""The figures of ``evaluate_tracks`` -- overview, rose graph, angle histogram, violin plots -- painted on the device.

Host mirror of the reference's module of this name (ysmr/plot_functions.py:29-257): the same three functions, the same
file names and figure size.  The reference hands the table to matplotlib, one ``scatter`` call per track; here the
columns go to HBM once, ``csrc/plots.hip`` paints the canvas, and the host stamps the lettering into the downloaded
canvas and writes the PNG (NumPy and zlib only); with ``png_on_device`` the canvas stays in HBM, ``csrc/png.hip`` stamps
the lettering and deflates the scanlines, and only the finished zlib stream is downloaded.  The image is this
project's own rendering of the same data -- which pixel a row lands on, which track wins a pixel and what colour it has are fixed by rules ("The figures"),
matplotlib's antialiased output is not reproduced; the lettering is a 5 x 7 bitmap font.  ``violin_plot`` is upstream's
function of that name (plot_functions.py:260-370) without seaborn: the categories, order statistics, moments and the
Gaussian kernel density estimate come from ``csrc/violin.hip``, which paints the canvas as well; ``evaluate_tracks``
calls it when the settings hold a true 'hip violin plots'.
"""
from __future__ import annotations

import ctypes
import logging
import math
import struct
import zlib

import numpy as np

from . import _lib

__all__ = ["angle_distribution_plot", "large_xy_plot", "rose_graph"]

FIG_INCHES = (11.6929133858, 8.2677165354)     # A4 landscape, as upstream: 3507 x 2480 at 300 dpi
MAX_TICKS = 32


# ---- PNG -------------------------------------------------------------------------------------------------------------

def write_png(path, rgb, dpi=300):
    """``rgb``: u8 [H, W, 3].  8-bit RGB, filter 0 on every row, zlib level 1, a pHYs chunk with ``dpi``."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("rgb must be [H, W, 3] with H, W >= 1, got {}".format(rgb.shape))
    h, w = rgb.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), np.uint8)              # a filter byte (0: none) in front of every row
    raw[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    per_metre = int(round(dpi / 0.0254))
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n")
        fh.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        fh.write(chunk(b"pHYs", struct.pack(">IIB", per_metre, per_metre, 1)))
        fh.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), 1)))
        fh.write(chunk(b"IEND", b""))


def png_mode(png_on_device):
    """What ``png_on_device`` (and the settings key 'hip png on device') asks for: ``None`` -- the host writes the file;
    ``'fixed'`` -- any true value: ``ysmr_png_deflate``; ``'dynamic'`` -- the string 'dynamic' in any case:
    ``ysmr_png_deflate_dynamic``, the smaller file."""
    if isinstance(png_on_device, str) and png_on_device.strip().lower() == "dynamic":
        return "dynamic"
    return "fixed" if png_on_device else None


def device_deflate(rgb_device, dynamic=False):
    """``ysmr_png_deflate`` of a u8 [H, W, 3] device tensor: the zlib stream of its PNG scanlines as bytes.  One launch
    chain; the 8-byte length is downloaded, then the stream.  ``dynamic``: ``ysmr_png_deflate_dynamic`` instead -- one
    block in a dynamic Huffman code, matches at four distances: a smaller stream of the same scanlines."""
    import torch
    if rgb_device.dtype != torch.uint8 or rgb_device.dim() != 3 or rgb_device.shape[2] != 3 or not rgb_device.is_contiguous():
        raise ValueError("rgb_device must be a contiguous u8 [H, W, 3] tensor, got {} {}".format(rgb_device.dtype, tuple(rgb_device.shape)))
    L = _lib.lib()
    dev = rgb_device.device
    h, w = int(rgb_device.shape[0]), int(rgb_device.shape[1])
    with _lib.on(dev):
        if dynamic:
            name, deflate = "ysmr_png_deflate_dynamic", L.ysmr_png_deflate_dynamic
            ws_bytes, out_bytes = L.ysmr_png_dynamic_workspace_bytes(w, h), L.ysmr_png_dynamic_stream_bytes_max(w, h)
        else:
            name, deflate = "ysmr_png_deflate", L.ysmr_png_deflate
            ws_bytes, out_bytes = L.ysmr_png_workspace_bytes(w, h), L.ysmr_png_stream_bytes_max(w, h)
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
        out = torch.empty(max(out_bytes, 256), dtype=torch.uint8, device=dev)
        length = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(deflate(_lib.stream_ptr(dev), rgb_device.data_ptr(), w, h, ws.data_ptr(), ws.numel(), out.data_ptr(),
                           out.numel(), length.data_ptr()), name)
        n = int(length.item())
        return out[:n].cpu().numpy().tobytes()


def write_png_device(path, rgb_device, dpi=300, dynamic=False):
    """``write_png`` for a canvas in HBM (u8 [H, W, 3] device tensor): the same chunks in the same layout, the IDAT body
    deflated on the device (``csrc/png.hip``: the fixed Huffman code, or with ``dynamic`` a dynamic one over matches at four
    distances) -- the file decodes to the same pixels, its bytes differ."""
    idat = device_deflate(rgb_device, dynamic)
    h, w = int(rgb_device.shape[0]), int(rgb_device.shape[1])

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    per_metre = int(round(dpi / 0.0254))
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n")
        fh.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        fh.write(chunk(b"pHYs", struct.pack(">IIB", per_metre, per_metre, 1)))
        fh.write(chunk(b"IDAT", idat))
        fh.write(chunk(b"IEND", b""))


# ---- lettering -------------------------------------------------------------------------------------------------------

# 5 x 7 glyphs of the printable ASCII characters, five column bytes each, bit 0 = top row (the classic LCD layout)
_FONT_HEX = (
    "0000000000" "00005f0000" "0007000700" "147f147f14" "242a7f2a12" "2313086462" "3649552250" "0005030000"
    "001c224100" "0041221c00" "14083e0814" "08083e0808" "0050300000" "0808080808" "0060600000" "2010080402"
    "3e5149453e" "00427f4000" "4261514946" "2141454b31" "1814127f10" "2745454539" "3c4a494930" "0171090503"
    "3649494936" "064949291e" "0036360000" "0056360000" "0814224100" "1414141414" "0041221408" "0201510906"
    "324979413e" "7e1111117e" "7f49494936" "3e41414122" "7f4141221c" "7f49494941" "7f09090901" "3e4149497a"
    "7f0808087f" "00417f4100" "2040413f01" "7f08142241" "7f40404040" "7f020c027f" "7f0408107f" "3e4141413e"
    "7f09090906" "3e4151215e" "7f09192946" "4649494931" "01017f0101" "3f4040403f" "1f2040201f" "3f4038403f"
    "6314081463" "0708700807" "6151494543" "007f414100" "0204081020" "0041417f00" "0402010204" "4040404040"
    "0001020400" "2054545478" "7f48444438" "3844444420" "384444487f" "3854545418" "087e090102" "0c5252523e"
    "7f08040478" "00447d4000" "2040443d00" "7f10284400" "00417f4000" "7c04180478" "7c08040478" "3844444438"
    "7c14141408" "081414187c" "7c08040408" "4854545420" "043f444020" "3c4040207c" "1c2040201c" "3c4030403c"
    "4428102844" "0c5050503c" "4464544c44" "0008364100" "00007f0000" "0041360800" "0804081008")
_MICRO = "7e2020103e"       # 'µ'
GLYPH_W, GLYPH_H, GLYPH_STEP = 5, 7, 6


def _glyph_table():
    def bitmap(hex10):
        cols = np.frombuffer(bytes.fromhex(hex10), np.uint8)
        return ((cols[None, :] >> np.arange(GLYPH_H)[:, None]) & 1).astype(bool)       # [row, column]
    table = {chr(32 + k): bitmap(_FONT_HEX[10 * k:10 * k + 10]) for k in range(95)}
    table["µ"] = bitmap(_MICRO)
    return table


_GLYPHS = _glyph_table()


def text_bitmap(text, scale=1):
    """bool [7 scale, 6 scale len(text) - scale]: the text in the 5 x 7 font, a column of space between characters;
    characters the font does not have become '?'."""
    text = str(text)
    out = np.zeros((GLYPH_H, max(GLYPH_STEP * len(text) - 1, 0)), bool)
    for k, ch in enumerate(text):
        out[:, GLYPH_STEP * k:GLYPH_STEP * k + GLYPH_W] = _GLYPHS.get(ch, _GLYPHS["?"])
    scale = max(1, int(scale))
    return np.repeat(np.repeat(out, scale, axis=0), scale, axis=1)


def text_size(text, scale=1):
    return max(GLYPH_STEP * len(str(text)) - 1, 0) * max(1, int(scale)), GLYPH_H * max(1, int(scale))


class StampList:
    """Stands in for the canvas in ``stamp_text`` / ``stamp_text_vertical`` and the ``decorate_*`` functions: the bitmaps
    are recorded instead of painted, for ``ysmr_plot_stamp`` to paint them into the canvas in HBM.  ``shape`` is the
    canvas' [H, W, 3]."""

    def __init__(self, height, width):
        self.shape = (int(height), int(width), 3)
        self.records = []          # (x, y, w, h, bit offset, colour)
        self._bits = []
        self._n_bits = 0

    def add(self, x, y, bm, colour):
        th, tw = bm.shape
        if th < 1 or tw < 1:
            return
        r, g, b = (int(c) & 255 for c in colour)
        self.records.append((int(x), int(y), tw, th, self._n_bits, r | g << 8 | b << 16))
        packed = np.packbits(np.ascontiguousarray(bm, dtype=bool).reshape(-1), bitorder="little")
        self._bits.append(packed)
        self._n_bits += 8 * len(packed)        # every bitmap starts on a byte

    def arrays(self):
        """(records as ``_lib.STAMP_DTYPE``, packed bits u8)"""
        rec = np.array(self.records, dtype=np.int64).reshape(-1, 6)
        out = np.zeros(len(rec), _lib.STAMP_DTYPE)
        for k, name in enumerate(_lib.STAMP_DTYPE.names):
            out[name] = rec[:, k]
        return out, np.concatenate(self._bits) if self._bits else np.zeros(0, np.uint8)


def _paint(rgb, x, y, bm, colour):
    """The set pixels of ``bm``, its top-left pixel at (x, y), in ``colour``; pixels outside the canvas are dropped."""
    if isinstance(rgb, StampList):
        rgb.add(x, y, bm, colour)
        return
    th, tw = bm.shape
    H, W = rgb.shape[:2]
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + tw, W), min(y + th, H)
    if x0 >= x1 or y0 >= y1:
        return
    rgb[y0:y1, x0:x1][bm[y0 - y:y1 - y, x0 - x:x1 - x]] = colour


def stamp_text(rgb, x, y, text, scale=1, colour=(0, 0, 0), anchor="left"):
    """Stamp ``text`` into ``rgb`` with the top-left pixel of its box at (x, y) -- or the box centred on / ending at x
    (anchor 'centre' / 'right').  Pixels outside the canvas are dropped.  ``rgb`` may be a ``StampList``."""
    bm = text_bitmap(text, scale)
    tw = bm.shape[1]
    x = int(x) - (tw // 2 if anchor == "centre" else tw if anchor == "right" else 0)
    _paint(rgb, x, int(y), bm, colour)


def device_stamp(rgb_device, stamps):
    """``ysmr_plot_stamp``: paints the records of a ``StampList`` into the canvas in HBM.  One upload carries the records
    and the bits."""
    import torch
    rec, bits = stamps.arrays()
    if not len(rec):
        return
    if tuple(rgb_device.shape) != tuple(stamps.shape) or rgb_device.dtype != torch.uint8 or not rgb_device.is_contiguous():
        raise ValueError("the canvas must be a contiguous u8 {} tensor, got {} {}".format(stamps.shape, rgb_device.dtype,
                                                                                        tuple(rgb_device.shape)))
    dev = rgb_device.device
    head = rec.view(np.uint8).reshape(-1)
    both = torch.from_numpy(np.concatenate([head, bits])).to(dev)
    with _lib.on(dev):
        _lib.check(_lib.lib().ysmr_plot_stamp(_lib.stream_ptr(dev), rgb_device.data_ptr(), stamps.shape[1], stamps.shape[0],
                                              both.data_ptr(), len(rec), both.data_ptr() + len(head), len(bits)), "ysmr_plot_stamp")


# ---- ticks and the view ----------------------------------------------------------------------------------------------

def nice_step(span, target=8):
    """The smallest of 1, 2, 5 x 10^k that cuts ``span`` into at most ``target`` pieces."""
    if not (span > 0) or not math.isfinite(span):
        return 1.0
    raw = span / target
    mag = 10.0 ** math.floor(math.log10(raw))
    for m in (1.0, 2.0, 5.0, 10.0):
        if m * mag >= raw * (1 - 1e-12):
            return m * mag
    return 10.0 * mag


def ticks_125(lo, hi, step):
    """The multiples of ``step`` in [lo, hi], at most MAX_TICKS of them."""
    if not (hi >= lo) or not (step > 0):
        return np.zeros(0)
    k0, k1 = math.ceil(lo / step - 1e-9), math.floor(hi / step + 1e-9)
    k = np.arange(k0, k1 + 1, dtype=np.float64)[:MAX_TICKS]
    digits = max(0, -int(math.floor(math.log10(step))) + 1)
    return np.round(k * step, digits)


def canvas_size(dpi):
    return int(FIG_INCHES[0] * dpi), int(FIG_INCHES[1] * dpi)


def figure_layout(W, H):
    """(axes rectangle, colour bar rectangle) as (x, y, w, h): the inner area is upstream's GridSpec (5 % left and right,
    matplotlib's 12 % above and 11 % below), the axes its left 98 / 100, the bar its right 2 / 100 less a gap."""
    x0, x1, y0, y1 = int(round(0.05 * W)), int(round(0.95 * W)), int(round(0.12 * H)), int(round(0.89 * H))
    inner_w, inner_h = max(x1 - x0, 8), max(y1 - y0, 2)
    slot = inner_w * 98 // 100
    gap = max(2, inner_w // 100)
    bar_w = max(inner_w - slot - 1, 1)
    return (x0, y0, max(slot - gap, 1), inner_h), (x0 + inner_w - bar_w, y0, bar_w, inner_h)


def track_view(extent, mode, px, dpi=300, size=None):
    """``ysmr_plot_view`` of a track figure for the data extent (min u, max u, min v, max v), and its tick values.
    Equal aspect, 5 % margin around the extent; an empty or single-point extent gets a range of 1 around it."""
    W, H = size or canvas_size(dpi)
    (ax_x, ax_y, ax_w, ax_h), bar = figure_layout(W, H)
    lo_u, hi_u, lo_v, hi_v = (float(e) for e in extent)
    if not all(math.isfinite(e) for e in (lo_u, hi_u, lo_v, hi_v)) or hi_u < lo_u or hi_v < lo_v:
        lo_u, hi_u, lo_v, hi_v = 0.0, 1.0, 0.0, 1.0
    span_u, span_v = hi_u - lo_u, hi_v - lo_v
    if span_u == 0 and span_v == 0:
        span_u = span_v = 1.0
    upp = max(1.1 * span_u / ax_w, 1.1 * span_v / ax_h)
    if not (upp > 0) or not math.isfinite(upp):
        upp = 1.0 / ax_w
    u0 = 0.5 * (lo_u + hi_u) - 0.5 * upp * ax_w
    v0 = 0.5 * (lo_v + hi_v) - 0.5 * upp * ax_h
    scale = dpi / 300.0
    view = _lib.PlotView()
    view.px, view.u0, view.v0, view.units_per_pixel = float(px), u0, v0, upp
    view.mode, view.width, view.height = int(mode), W, H
    view.ax_x, view.ax_y, view.ax_w, view.ax_h = ax_x, ax_y, ax_w, ax_h
    # upstream's s=1 markers at 300 dpi: a '.' of about three pixels, an 'o' of about five
    view.r2_dot, view.r2_start = int(round(1 * scale * scale)), int(round(4 * scale * scale))
    view.bar_x, view.bar_y, view.bar_w, view.bar_h = bar
    step = nice_step(upp * ax_w)
    ticks_u, ticks_v = ticks_125(u0, u0 + upp * ax_w, step), ticks_125(v0, v0 + upp * ax_h, step)
    cols = [(t, ax_x + int(math.floor((t - u0) / upp))) for t in ticks_u]
    rows = [(t, ax_y + ax_h - 1 - int(math.floor((t - v0) / upp))) for t in ticks_v]
    cols = [(t, c) for t, c in cols if ax_x <= c < ax_x + ax_w]
    rows = [(t, r) for t, r in rows if ax_y <= r < ax_y + ax_h]
    view.n_grid_cols, view.n_grid_rows = len(cols), len(rows)
    for k, (_, c) in enumerate(cols):
        view.grid_cols[k] = c
    for k, (_, r) in enumerate(rows):
        view.grid_rows[k] = r
    return view, cols, rows


def _label(value):
    return "{:g}".format(value + 0.0)          # (+ 0.0: no '-0')


def decorate_track_figure(rgb, view, cols, rows, title, dist_min, dist_max, dpi=300):
    """Title, tick labels, 'µm' and the colour bar's labels, stamped outside the axes rectangle."""
    s = max(1, int(round(dpi / 100.0)))
    gap = 2 * s
    stamp_text(rgb, view.ax_x + view.ax_w // 2, view.ax_y - gap - GLYPH_H * (s + 1) - 1, title, s + 1, anchor="centre")
    below = view.ax_y + view.ax_h + 1 + gap
    for t, c in cols:
        stamp_text(rgb, c, below, _label(t), s, anchor="centre")
    stamp_text(rgb, view.ax_x + view.ax_w // 2, below + (GLYPH_H + 3) * s, "µm", s, anchor="centre")
    widest = 0
    for t, r in rows:
        stamp_text(rgb, view.ax_x - 1 - gap, r - GLYPH_H * s // 2, _label(t), s, anchor="right")
        widest = max(widest, text_size(_label(t), s)[0])
    stamp_text(rgb, view.ax_x - 1 - 2 * gap - widest, view.ax_y + view.ax_h // 2 - GLYPH_H * s // 2, "µm", s, anchor="right")
    if view.bar_w > 0:
        right = view.bar_x + view.bar_w + 1 + gap
        stamp_text(rgb, right, view.bar_y, "{:.4g}".format(dist_max), s)
        stamp_text(rgb, right, view.bar_y + view.bar_h - GLYPH_H * s, "{:.4g}".format(dist_min), s)
        stamp_text(rgb, right, view.bar_y + view.bar_h // 2 - GLYPH_H * s // 2, "µm", s)


# ---- the device calls ------------------------------------------------------------------------------------------------

def _upload(df, dev, moving=False):
    import torch
    ids = torch.from_numpy(np.ascontiguousarray(df["TRACK_ID"].to_numpy(), dtype=np.uint32).view(np.int32)).to(dev)
    x = torch.from_numpy(np.ascontiguousarray(df["POSITION_X"].to_numpy(), dtype=np.float64)).to(dev)
    y = torch.from_numpy(np.ascontiguousarray(df["POSITION_Y"].to_numpy(), dtype=np.float64)).to(dev)
    if moving:
        return ids, x, y, torch.from_numpy(np.ascontiguousarray(df["moving"].to_numpy(), dtype=np.int8)).to(dev)
    return ids, x, y


def device_extent(ids, x, y, mode, px, dev):
    """``ysmr_plot_extent`` on device columns: (min u, max u, min v, max v) as a NumPy array."""
    import torch
    out = torch.empty(4, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ysmr_plot_extent(_lib.stream_ptr(dev), ids.numel(), ids.data_ptr(), x.data_ptr(), y.data_ptr(), int(mode),
                                           float(px), out.data_ptr()), "ysmr_plot_extent")
    return out.cpu().numpy()


def device_tracks(ids, x, y, dist, view, dev, download=True):
    """``ysmr_plot_tracks`` on device columns (``dist``: the tracks' distances, a NumPy array): the canvas as u8
    [H, W, 3] on the host (``download=False``: the device tensor)."""
    import torch
    L = _lib.lib()
    dist = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    n, nt = ids.numel(), dist.numel()
    ws = torch.empty(max(L.ysmr_plot_workspace_bytes(n, nt, view.width, view.height), 256), dtype=torch.uint8, device=dev)
    rgb = torch.empty(view.height, view.width, 3, dtype=torch.uint8, device=dev)
    _lib.check(L.ysmr_plot_tracks(_lib.stream_ptr(dev), n, ids.data_ptr(), x.data_ptr(), y.data_ptr(), nt, dist.data_ptr(), 1,
                                  ctypes.byref(view), ws.data_ptr(), ws.numel(), rgb.data_ptr()), "ysmr_plot_tracks")
    return rgb.cpu().numpy() if download else rgb


def device_angle_histogram(ids, x, y, moving, lag, edges, dev):
    """``ysmr_plot_angle_histogram``: (counts int64 [bins], number of selected rows)."""
    import torch
    L = _lib.lib()
    n, n_bins = ids.numel(), len(edges) - 1
    e = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(dev)
    ws = torch.empty(max(L.ysmr_plot_workspace_bytes(n, 0, 0, 0), 256), dtype=torch.uint8, device=dev)
    out = torch.empty(max(n_bins, 1) + 1, dtype=torch.int64, device=dev)
    _lib.check(L.ysmr_plot_angle_histogram(_lib.stream_ptr(dev), n, ids.data_ptr(), x.data_ptr(), y.data_ptr(), moving.data_ptr(),
                                           int(lag), int(n_bins), e.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr() + 8,
                                           out.data_ptr()), "ysmr_plot_angle_histogram")
    host = out.cpu().numpy()
    return host[1:1 + n_bins].copy(), int(host[0])


def device_wedges(W, H, cx, cy, dirs, r2, ring_r2, dev, download=True):
    """``ysmr_plot_wedges``: the canvas as u8 [H, W, 3] on the host (``download=False``: the device tensor)."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64)).to(dev)
    r = torch.from_numpy(np.ascontiguousarray(r2, dtype=np.int64)).to(dev)
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().ysmr_plot_wedges(_lib.stream_ptr(dev), W, H, int(cx), int(cy), len(r2), d.data_ptr(), r.data_ptr(),
                                           int(ring_r2), rgb.data_ptr()), "ysmr_plot_wedges")
    return rgb.cpu().numpy() if download else rgb


def track_distances(df):
    """A track's travelled distance, per track in table order: what upstream's ``distance_colour`` is made of."""
    ids = df["TRACK_ID"].to_numpy()
    start = np.ones(len(ids), bool)
    start[1:] = ids[1:] != ids[:-1]
    return np.add.reduceat(df["travelled_dist"].to_numpy(dtype=np.float64), np.flatnonzero(start)) if len(ids) else np.zeros(0)


def _finish_figure(rgb, decorate, save_path, dpi, png_on_device):
    """Lettering and file.  ``decorate(canvas)`` stamps into a NumPy canvas -- or, with ``png_on_device`` (``rgb`` is the
    device tensor then), into a ``StampList`` that the device paints before it deflates the canvas; ``'dynamic'`` chooses
    the dynamic stream (``png_mode``)."""
    if png_on_device:
        stamps = StampList(rgb.shape[0], rgb.shape[1])
        decorate(stamps)
        device_stamp(rgb, stamps)
        write_png_device(save_path, rgb, dpi, dynamic=png_mode(png_on_device) == "dynamic")
    else:
        decorate(rgb)
        write_png(save_path, rgb, dpi)


def _track_figure(df, mode, plot_title_name, save_path, px, dist_min, dist_max, dpi, device, distances, png_on_device=False):
    import torch
    logger = logging.getLogger("ysmr").getChild(__name__)
    dev = torch.device(device)
    dist = np.ascontiguousarray(track_distances(df) if distances is None else distances, dtype=np.float64)
    if not dist_max:
        dist_max = float(dist.max()) if len(dist) else 0.0
    with _lib.on(dev):
        ids, x, y = _upload(df, dev)
        view, cols, rows = track_view(device_extent(ids, x, y, mode, px, dev), mode, px, dpi)
        rgb = device_tracks(ids, x, y, dist, view, dev, download=False) if png_on_device else device_tracks(ids, x, y, dist, view, dev)
    _finish_figure(rgb, lambda canvas: decorate_track_figure(canvas, view, cols, rows, plot_title_name, dist_min, dist_max, dpi),
                   save_path, dpi, png_on_device)
    logger.debug("Saving figure {}".format(save_path))


def large_xy_plot(df, plot_title_name, save_path, px_to_micrometre=1, dist_min=0, dist_max=None, dpi=300, device="cuda:0",
                  distances=None, png_on_device=False):
    """Every track's path on one plot, black dots where the tracks start (plot_functions.py:109-188).  ``distances``:
    the tracks' 'Distance (µm)' in table order (default: the sums of the table's 'travelled_dist').  ``png_on_device``:
    lettering and deflate on the device, the canvas is not downloaded -- ``True``: one block in the fixed Huffman code;
    ``'dynamic'``: one block in a dynamic code over matches at four distances, the smaller file (``png_mode``).  The same
    two values are taken by ``rose_graph``, ``angle_distribution_plot`` and ``violin_plot``."""
    _track_figure(df, 0, plot_title_name, save_path, px_to_micrometre, dist_min, dist_max, dpi, device, distances, png_on_device)


def rose_graph(df, plot_title_name, save_path, dist_min=0, dist_max=None, dpi=300, device="cuda:0", distances=None,
               px_to_micrometre=1, png_on_device=False):
    """Every track's path from a common origin (plot_functions.py:191-257).  Upstream reads its 'x_norm' / 'y_norm'
    columns; here they are formed from POSITION_X / POSITION_Y and ``px_to_micrometre`` on the device."""
    _track_figure(df, 1, plot_title_name, save_path, px_to_micrometre, dist_min, dist_max, dpi, device, distances, png_on_device)


def wedge_plan(counts, W, H):
    """Centre, ring and bar radii (squared, exact integers) of the polar chart: the longest bar reaches the ring."""
    cx, cy = W // 2, int(round(0.53 * H))
    ring = max(1, int(0.40 * min(W, H)))
    top = int(max(counts)) if len(counts) else 0
    r2 = [(ring * ring * int(c) * int(c)) // (top * top) if top else 0 for c in counts]
    return cx, cy, ring * ring, r2


def wedge_boundaries(edges):
    """Boundary directions (east, north) for ``ysmr_plot_wedges`` and the bin of every wedge.  A bar must be narrower
    than half a turn, so fewer than three bins are drawn with their bars cut in sectors."""
    edges = np.asarray(edges, np.float64)
    n_bins = len(edges) - 1
    parts = 1 if n_bins >= 3 else 3 if n_bins == 1 else 2
    fine = np.concatenate([np.linspace(edges[k], edges[k + 1], parts + 1)[:-1] for k in range(n_bins)] + [edges[-1:]])
    dirs = np.stack([np.sin(fine), np.cos(fine)], axis=1)
    dirs[-1] = dirs[0]                                      # one full turn: the seam is one direction, bit for bit
    return np.ascontiguousarray(dirs), np.repeat(np.arange(n_bins), parts)


def decorate_angle_figure(rgb, W, H, cx, cy, ring_r2, title, n_points, top, dpi=300):
    """Title with the number of points, the four compass labels and the longest bar's count at the ring."""
    s = max(1, int(round(dpi / 100.0)))
    ring = math.isqrt(ring_r2)
    stamp_text(rgb, W // 2, int(round(0.05 * H)), "{} Data points: {}".format(title, n_points), s + 1, anchor="centre")
    stamp_text(rgb, cx, cy - ring - (GLYPH_H + 2) * s, "0", s, anchor="centre")
    stamp_text(rgb, cx + ring + 2 * s, cy - GLYPH_H * s // 2, "90", s)
    stamp_text(rgb, cx, cy + ring + 2 * s, "180", s, anchor="centre")
    stamp_text(rgb, cx - ring - 2 * s, cy - GLYPH_H * s // 2, "270", s, anchor="right")
    stamp_text(rgb, cx + int(0.71 * ring) + 2 * s, cy - int(0.71 * ring) - (GLYPH_H + 2) * s, str(int(top)), s)


def angle_distribution_plot(df, bins_number, plot_title_name, save_path, dpi=300, compare_n_frames=10, device="cuda:0",
                            png_on_device=False):
    """Polar histogram of the headings of the moving rows of tracks that move more than 70 % of the time
    (plot_functions.py:29-90).  The table evaluate_tracks returns holds the folded change of heading in degrees, not the
    heading, so the heading is formed again from POSITION_X / POSITION_Y with the lag ``compare_n_frames``."""
    import torch
    logger = logging.getLogger("ysmr").getChild(__name__)
    dev = torch.device(device)
    bins_number = int(bins_number)
    edges = np.linspace(-np.pi, np.pi, bins_number + 1)
    W, H = canvas_size(dpi)
    with _lib.on(dev):
        ids, x, y, moving = _upload(df, dev, moving=True)
        counts, n_points = device_angle_histogram(ids, x, y, moving, compare_n_frames, edges, dev)
        if not n_points:
            logger.warning("Cannot create angle distribution plot as there are no motile tracks.")
            return
        dirs, bin_of = wedge_boundaries(edges)
        cx, cy, ring_r2, r2 = wedge_plan(counts[bin_of], W, H)
        rgb = device_wedges(W, H, cx, cy, dirs, r2, ring_r2, dev, download=False) if png_on_device else device_wedges(W, H, cx, cy, dirs, r2, ring_r2, dev)
    _finish_figure(rgb, lambda canvas: decorate_angle_figure(canvas, W, H, cx, cy, ring_r2, plot_title_name, n_points, counts.max(), dpi),
                   save_path, dpi, png_on_device)
    logger.debug("Saving figure {}".format(save_path))


# ---- the violin plots ------------------------------------------------------------------------------------------------

VIOLIN_INCHES = (11.6929133858 / 2, 8.2677165354 / 2)     # half A4 landscape, as upstream: 1753 x 1240 at 300 dpi


def violin_canvas_size(dpi):
    return int(VIOLIN_INCHES[0] * dpi), int(VIOLIN_INCHES[1] * dpi)


def violin_layout(W, H):
    """The axes rectangle (x, y, w, h): room for the tick labels and the column's name on the left, for the title and the
    three lines of the text boxes above, for the category names below."""
    x0, x1, y0, y1 = int(round(0.11 * W)), int(round(0.97 * W)), int(round(0.17 * H)), int(round(0.90 * H))
    return x0, y0, max(x1 - x0, 1), max(y1 - y0, 1)


def device_violin_stats(cut, value, lo, hi, dev):
    """``ysmr_violin_stats``: (summaries as a NumPy record array [len(lo) + 1] of ``_lib.VIOLIN_SUMMARY_DTYPE``,
    densities f64 [len(lo) + 1, 100]); violin 0 is 'All'."""
    import torch
    L = _lib.lib()
    cut = torch.from_numpy(np.ascontiguousarray(cut, dtype=np.float64)).to(dev)
    value = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(dev)
    n, n_cuts = cut.numel(), len(lo)
    if value.numel() != n or len(hi) != n_cuts:
        raise ValueError("cut and value, lo and hi must have the same lengths")
    if n_cuts > _lib.VIOLIN_MAX_CUTS:
        raise ValueError("at most {} intervals, got {}".format(_lib.VIOLIN_MAX_CUTS, n_cuts))
    bounds = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(lo, np.float64), np.asarray(hi, np.float64)]))).to(dev)
    ws = torch.empty(max(L.ysmr_violin_workspace_bytes(n, n_cuts + 1, 0), 256), dtype=torch.uint8, device=dev)
    size = _lib.VIOLIN_SUMMARY_DTYPE.itemsize
    sums = torch.empty((n_cuts + 1) * size, dtype=torch.uint8, device=dev)
    dens = torch.empty(n_cuts + 1, _lib.VIOLIN_GRID, dtype=torch.float64, device=dev)
    _lib.check(L.ysmr_violin_stats(_lib.stream_ptr(dev), n, cut.data_ptr(), 1, value.data_ptr(), 1, n_cuts, bounds.data_ptr(),
                                   bounds.data_ptr() + 8 * n_cuts, ws.data_ptr(), ws.numel(), sums.data_ptr(), dens.data_ptr()),
               "ysmr_violin_stats")
    return sums.cpu().numpy().view(_lib.VIOLIN_SUMMARY_DTYPE).copy(), dens.cpu().numpy()


def device_violins(sums, dens, view, dev, download=True):
    """``ysmr_plot_violins`` on summaries and densities given as NumPy arrays: the canvas as u8 [H, W, 3] on the host
    (``download=False``: the device tensor)."""
    import torch
    L = _lib.lib()
    n = int(view.n_violins)
    sums = np.ascontiguousarray(sums, dtype=_lib.VIOLIN_SUMMARY_DTYPE)
    dens = np.ascontiguousarray(dens, dtype=np.float64)
    if len(sums) != n or dens.shape != (n, _lib.VIOLIN_GRID):
        raise ValueError("the view has {} violins, the summaries {}, the densities {}".format(n, len(sums), dens.shape))
    s = torch.from_numpy(sums.view(np.uint8).copy()).to(dev)
    d = torch.from_numpy(dens).to(dev)
    ws = torch.empty(max(L.ysmr_violin_workspace_bytes(0, n, view.ax_h), 256), dtype=torch.uint8, device=dev)
    rgb = torch.empty(view.height, view.width, 3, dtype=torch.uint8, device=dev)
    _lib.check(L.ysmr_plot_violins(_lib.stream_ptr(dev), n, s.data_ptr(), d.data_ptr(), ctypes.byref(view), ws.data_ptr(), ws.numel(),
                                   rgb.data_ptr()), "ysmr_plot_violins")
    return rgb.cpu().numpy() if download else rgb


def violin_view(sums, y_min=None, y_max=None, dpi=300, size=None):
    """``ysmr_violin_view`` for the summaries of one figure and its y ticks as (value, canvas row) pairs.  A limit that is
    None or False is automatic: the 'All' violin's minimum / maximum with a margin of 5 % of its range.  The violins that
    exist (values > 0) share the axes' width in order, as seaborn's categorical axis does."""
    W, H = size or violin_canvas_size(dpi)
    ax_x, ax_y, ax_w, ax_h = violin_layout(W, H)
    n = len(sums)
    if not 1 <= n <= _lib.VIOLIN_MAX_SLOTS:
        raise ValueError("a figure holds 1..{} violins, got {}".format(_lib.VIOLIN_MAX_SLOTS, n))
    vmin, vmax = (float(sums[0]["vmin"]), float(sums[0]["vmax"])) if sums[0]["values"] > 0 else (0.0, 1.0)
    margin = 0.05 * (vmax - vmin) if vmax > vmin else 0.5
    lo = vmin - margin if y_min is None or y_min is False else float(y_min)
    hi = vmax + margin if y_max is None or y_max is False else float(y_max)
    if not (math.isfinite(lo) and math.isfinite(hi)) or not hi > lo:
        hi = lo + 1.0 if math.isfinite(lo) else 1.0
        lo = lo if math.isfinite(lo) else 0.0
    view = _lib.ViolinView()
    view.y0, view.units_per_pixel = lo, (hi - lo) / ax_h
    view.width, view.height, view.ax_x, view.ax_y, view.ax_w, view.ax_h = W, H, ax_x, ax_y, ax_w, ax_h
    view.n_violins = n
    # upstream's linewidth 1 and seaborn's inner box at 300 dpi: a line of 3 pixels, a box of 13, a dot of radius 4
    s = max(1, int(round(dpi / 100.0)))
    view.line_half, view.box_half, view.dot_r2 = s // 2, 2 * s, (s + 1) * (s + 1)
    drawn = [v for v in range(n) if sums[v]["values"] > 0]
    for pos, v in enumerate(drawn):
        left, right = ax_x + pos * ax_w // len(drawn), ax_x + (pos + 1) * ax_w // len(drawn)
        view.slot_x[v], view.slot_w[v], view.slot_colour[v] = left, right - left, pos
    ticks = ticks_125(lo, hi, nice_step(hi - lo))
    rows = [(t, ax_y + ax_h - 1 - int(math.floor((t - lo) / view.units_per_pixel))) for t in ticks]
    rows = [(t, r) for t, r in rows if ax_y <= r < ax_y + ax_h]
    view.n_grid_rows = len(rows)
    for k, (_, r) in enumerate(rows):
        view.grid_rows[k] = r
    return view, rows


def violin_text_boxes(sums, labels):
    """Upstream's text box of every violin that exists: (violin, text) in cut-list order."""
    total = int(sums[0]["members"])
    boxes = []
    for v, label in enumerate(labels):
        if not sums[v]["values"] > 0:
            continue
        share = "{:.1%}".format(int(sums[v]["members"]) / total) if total > 0 else "error"
        boxes.append((v, "{}: {} ({})\nMedian: {:.2f}\nAverage:  {:.2f}".format(label, int(sums[v]["members"]), share,
                                                                               float(sums[v]["q50"]), float(sums[v]["mean"]))))
    return boxes


def _fitting_scale(texts, room, largest):
    """The largest lettering scale <= ``largest`` at which every text is at most ``room`` pixels wide (1 if none is)."""
    for s in range(max(1, largest), 1, -1):
        if all(text_size(t, s)[0] <= room for t in texts):
            return s
    return 1


def stamp_text_vertical(rgb, x, y, text, scale=1, colour=(0, 0, 0)):
    """``text`` reading upwards, its box centred on row ``y`` with its left edge at column ``x``; clipped like stamp_text."""
    bm = np.rot90(text_bitmap(text, scale))
    _paint(rgb, int(x), int(y) - bm.shape[0] // 2, bm, colour)


def decorate_violin_figure(rgb, view, rows, title, column, labels, boxes, dpi=300):
    """Title, tick labels, the column's name along y, the category names under the violins and the text boxes above them,
    all stamped outside the axes rectangle."""
    s = max(1, int(round(dpi / 150.0)))
    gap = 2 * s
    ax_x, ax_y, ax_w, ax_h = view.ax_x, view.ax_y, view.ax_w, view.ax_h
    stamp_text(rgb, ax_x + ax_w // 2, max(gap, int(round(0.015 * view.height))), title, s + 1, anchor="centre")
    widest = 0
    for t, r in rows:
        stamp_text(rgb, ax_x - 1 - gap, r - GLYPH_H * s // 2, _label(t), s, anchor="right")
        widest = max(widest, text_size(_label(t), s)[0])
    stamp_text_vertical(rgb, max(gap, ax_x - 1 - 3 * gap - widest - GLYPH_H * s), ax_y + ax_h // 2, column, s)
    if boxes:
        room = ax_w // len(boxes) - int(0.02 * ax_w)
        sb = _fitting_scale([line for _, text in boxes for line in text.split("\n")], room, s)
        line_h = (GLYPH_H + 2) * sb
        for idx, (v, text) in enumerate(boxes):
            lines = text.split("\n")
            for k, line in enumerate(lines):
                stamp_text(rgb, ax_x + idx * ax_w // len(boxes) + int(0.015 * ax_w), ax_y - gap - line_h * (len(lines) - k), line, sb)
        sl = _fitting_scale([labels[v] for v, _ in boxes], room, s)
        for v, _ in boxes:
            stamp_text(rgb, view.slot_x[v] + view.slot_w[v] // 2, ax_y + ax_h + 1 + 2 * gap, labels[v], sl, anchor="centre")


def _cut_column(df, cut_off_category):
    name = str(cut_off_category)
    if name.startswith("Categories (") and name.endswith(")") and name[len("Categories ("):-1] in df.columns:
        return name[len("Categories ("):-1]
    raise ValueError("cannot tell the column the categories are cut on from {!r}".format(cut_off_category))


def violin_plot(df, save_path, category, cut_off_category, cut_off_list, plot_title_name="\n\n", y_min=None, y_max=None, dpi=300,
                device="cuda:0", png_on_device=False):
    """One violin per entry of ``cut_off_list`` -- (low, high, name) triples, 'All' in front -- of the column
    ``category`` of the per-track table ``df`` (plot_functions.py:260-370).  Upstream receives the table with a label
    column made on the host; here ``cut_off_category`` ('Categories (<column>)') names the column the intervals cut,
    and the device tells the tracks apart."""
    import torch
    logger = logging.getLogger("ysmr").getChild(__name__)
    dev = torch.device(device)
    cut = df[_cut_column(df, cut_off_category)].to_numpy(dtype=np.float64)
    value = df[category].to_numpy(dtype=np.float64)
    labels = [str(name) for _, _, name in cut_off_list]
    lo, hi = [float(a) for a, _, _ in cut_off_list[1:]], [float(b) for _, b, _ in cut_off_list[1:]]
    with _lib.on(dev):
        sums, dens = device_violin_stats(cut, value, lo, hi, dev)
        view, rows = violin_view(sums, y_min, y_max, dpi)
        rgb = device_violins(sums, dens, view, dev, download=False) if png_on_device else device_violins(sums, dens, view, dev)
    boxes = violin_text_boxes(sums, labels)
    _finish_figure(rgb, lambda canvas: decorate_violin_figure(canvas, view, rows, str(plot_title_name).strip(), category, labels, boxes, dpi),
                   save_path, dpi, png_on_device)
    logger.debug("Saving figure {}".format(save_path))
