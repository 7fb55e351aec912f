"""NumPy model of the violin plots (csrc/violin.hip; DESIGN.md, "The figures"): the split into categories, the per-violin
summaries, the Gaussian kernel density estimate, the profile and the sequential painter.  Sums are ``math.fsum`` (exact,
then rounded once): what the device's fixed-order sums are measured against."""
import math

import numpy as np

GRID = 100
SQRT_2PI = 2.5066282746310002
WHITE, GREY, INNER, BLACK = (255, 255, 255), (176, 176, 176), (76, 76, 76), (0, 0, 0)
FILL = [(76, 114, 176), (221, 132, 82), (85, 168, 104), (196, 78, 82), (129, 114, 179), (147, 120, 96), (218, 139, 195),
        (140, 140, 140), (204, 185, 116), (100, 181, 205)]
SUMMARY_DTYPE = np.dtype([("members", "<i8"), ("values", "<i8")] + [(k, "<f8") for k in (
    "vmin", "vmax", "q25", "q50", "q75", "whisker_lo", "whisker_hi", "mean", "h")])
ROW_CLAMP = 1048576.0


# ---- categories ------------------------------------------------------------------------------------------------------

def categories(cut, lo, hi):
    """Per track the violin beyond 'All' it belongs to (k + 1 for the LAST interval k with lo_k <= c < hi_k), 0: none."""
    cut = np.asarray(cut, np.float64)
    cat = np.zeros(len(cut), np.int64)
    for k, (a, b) in enumerate(zip(lo, hi)):
        with np.errstate(invalid="ignore"):
            cat[(np.float64(a) <= cut) & (cut < np.float64(b))] = k + 1
    return cat


def violin_values(cut, value, lo, hi):
    """[(members, sorted finite values)] for 'All' and every interval."""
    value = np.asarray(value, np.float64)
    cat = categories(cut, lo, hi)
    out = []
    for v in range(len(lo) + 1):
        mine = value if v == 0 else value[cat == v]
        out.append((len(mine), np.sort(mine[np.isfinite(mine)])))
    return out


# ---- summaries -------------------------------------------------------------------------------------------------------

def quartile(x, q):
    """NumPy's linear rule on sorted x."""
    n = len(x)
    pos = np.float64(q) * np.float64(n - 1)
    lo = int(math.floor(pos))
    t = pos - np.float64(lo)
    a, b = np.float64(x[lo]), np.float64(x[min(lo + 1, n - 1)])
    return a + (b - a) * t if t < 0.5 else b - (b - a) * (np.float64(1.0) - t)


def summary(members, x):
    """One SUMMARY_DTYPE record of the sorted finite values ``x``."""
    s = np.zeros((), SUMMARY_DTYPE)
    n = len(x)
    s["members"], s["values"] = members, n
    if n == 0:
        return s
    x = np.asarray(x, np.float64)
    s["vmin"], s["vmax"] = x[0], x[-1]
    q25, q50, q75 = (quartile(x, q) for q in (0.25, 0.5, 0.75))
    s["q25"], s["q50"], s["q75"] = q25, q50, q75
    iqr = q75 - q25
    fence_lo, fence_hi = q25 - np.float64(1.5) * iqr, q75 + np.float64(1.5) * iqr
    s["whisker_lo"] = x[x >= fence_lo][0]
    s["whisker_hi"] = x[x <= fence_hi][-1]
    mean = math.fsum(x) / n
    s["mean"] = mean
    s["h"] = 0.2 * math.sqrt(math.fsum((float(v) - mean) ** 2 for v in x) / (n - 1)) if n >= 2 else 0.0
    return s


def grid_points(vmin, vmax):
    step = (np.float64(vmax) - np.float64(vmin)) / np.float64(GRID - 1)
    g = np.float64(vmin) + np.arange(GRID, dtype=np.float64) * step
    g[-1] = vmax
    return g


def density(x, s):
    """d_j of the formula; zeros for a violin without a density (values < 2 or h == 0)."""
    n, h = int(s["values"]), float(s["h"])
    if n < 2 or not (h > 0.0):
        return np.zeros(GRID)
    x = np.asarray(x, np.float64)
    norm = 1.0 / (n * h * SQRT_2PI)
    out = np.zeros(GRID)
    for j, g in enumerate(grid_points(s["vmin"], s["vmax"])):
        z = (g - x) / h
        out[j] = norm * math.fsum(np.exp(-0.5 * z * z))
    return out


def stats(cut, value, lo, hi):
    """(summaries SUMMARY_DTYPE [violins], densities f64 [violins, 100])."""
    groups = violin_values(cut, value, lo, hi)
    sums = np.zeros(len(groups), SUMMARY_DTYPE)
    dens = np.zeros((len(groups), GRID))
    for v, (members, x) in enumerate(groups):
        sums[v] = summary(members, x)
        dens[v] = density(x, sums[v])
    return sums, dens


# ---- the painter -----------------------------------------------------------------------------------------------------

def make_view(W, H, ax, y0, upp, slot_x, slot_w, slot_colour=None, grid_rows=(), line_half=1, box_half=3, dot_r2=4):
    return dict(W=W, H=H, ax=tuple(ax), y0=float(y0), upp=float(upp), slot_x=list(slot_x), slot_w=list(slot_w),
                slot_colour=list(slot_colour) if slot_colour is not None else list(range(len(slot_x))), grid_rows=list(grid_rows),
                line_half=line_half, box_half=box_half, dot_r2=dot_r2)


def to_struct(view):
    from ysmr_amd import _lib
    v = _lib.ViolinView()
    v.y0, v.units_per_pixel, v.width, v.height = view["y0"], view["upp"], view["W"], view["H"]
    v.ax_x, v.ax_y, v.ax_w, v.ax_h = view["ax"]
    v.n_violins, v.n_grid_rows = len(view["slot_x"]), len(view["grid_rows"])
    v.line_half, v.box_half, v.dot_r2 = view["line_half"], view["box_half"], view["dot_r2"]
    for k, r in enumerate(view["grid_rows"]):
        v.grid_rows[k] = r
    for k in range(len(view["slot_x"])):
        v.slot_x[k], v.slot_w[k], v.slot_colour[k] = view["slot_x"][k], view["slot_w"][k], view["slot_colour"][k]
    return v


def from_struct(v):
    return make_view(v.width, v.height, (v.ax_x, v.ax_y, v.ax_w, v.ax_h), v.y0, v.units_per_pixel, list(v.slot_x[:v.n_violins]),
                     list(v.slot_w[:v.n_violins]), list(v.slot_colour[:v.n_violins]), list(v.grid_rows[:v.n_grid_rows]),
                     v.line_half, v.box_half, v.dot_r2)


def row_of(value, view):
    ax_h = view["ax"][3]
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.float64(value) - np.float64(view["y0"])) / np.float64(view["upp"]))
    if not (f >= -ROW_CLAMP):
        f = -ROW_CLAMP
    if f > ROW_CLAMP:
        f = ROW_CLAMP
    return ax_h - 1 - int(f)


def profile(sums, dens, view):
    """(half widths int32 [violins, ax_h], marks int32 [violins, 8]) as k_vi_profile writes them."""
    ax_h = view["ax"][3]
    n = len(view["slot_x"])
    prof = np.full((n, ax_h), -1, np.int32)
    marks = np.zeros((n, 8), np.int32)
    max_values = max([int(sums[u]["values"]) for u in range(n) if view["slot_w"][u] > 0] + [0])
    r = np.arange(ax_h)
    y = np.float64(view["y0"]) + ((ax_h - 1 - r).astype(np.float64) + 0.5) * np.float64(view["upp"])
    for w in range(n):
        s, d = sums[w], np.asarray(dens[w], np.float64)
        peak = max(0.0, float(d.max()))
        drawn = view["slot_w"][w] > 0 and s["values"] > 0
        line = drawn and (s["values"] == 1 or not (s["h"] > 0.0))
        body = drawn and not line and peak > 0.0 and s["vmax"] > s["vmin"]
        if body:
            step = (s["vmax"] - s["vmin"]) / np.float64(GRID - 1)
            inside = (y >= s["vmin"]) & (y <= s["vmax"])
            p = (y[inside] - s["vmin"]) / step
            j = np.clip(np.floor(p).astype(np.int64), 0, GRID - 2)
            t = p - j.astype(np.float64)
            dd = d[j] + (d[j + 1] - d[j]) * t
            a = dd / np.float64(peak)
            a = a * np.float64(int(s["values"]))
            a = a / np.float64(max_values)
            a = a * np.float64(0.95)
            a = a * np.float64(view["slot_w"][w])
            a = a / np.float64(2.0)
            a = np.floor(a)
            prof[w, inside] = np.where(a >= 0.0, np.minimum(a, 65536.0), -1.0).astype(np.int32)
        marks[w] = [1 if body else 2 if line else 0, row_of(s["q50"], view), row_of(s["q25"], view), row_of(s["q75"], view),
                    row_of(s["whisker_lo"], view), row_of(s["whisker_hi"], view), row_of(s["vmin"], view), 0]
    return prof, marks


def paint(prof, marks, view):
    """The sequential painter: layer after layer, later over earlier.  u8 [H, W, 3]."""
    W, H = view["W"], view["H"]
    ax_x, ax_y, ax_w, ax_h = view["ax"]
    rgb = np.full((H, W, 3), 255, np.uint8)
    axes = rgb[ax_y:ax_y + ax_h, ax_x:ax_x + ax_w]                       # a view: painting it paints the canvas
    for r in view["grid_rows"]:
        if ax_y <= r < ax_y + ax_h:
            axes[r - ax_y, :] = GREY
    rows = np.arange(ax_h)[:, None]
    taken = np.zeros(ax_w, bool)                                          # (a column belongs to the lowest slot that holds it)
    for w in range(len(view["slot_x"])):
        sw, sx = view["slot_w"][w], view["slot_x"][w] - ax_x
        if sw <= 0:
            continue
        cols = np.arange(sx, sx + sw)
        cols = cols[~taken[cols]]
        taken[cols] = True
        kind = marks[w][0]
        if kind == 0 or len(cols) == 0:
            continue
        cx = sx + sw // 2
        dx = (np.arange(ax_w) - cx)[None, :]
        in_slot = np.zeros((1, ax_w), bool)
        in_slot[0, cols] = True
        m = marks[w]
        if kind == 1:
            fill = in_slot & (np.abs(dx) <= prof[w][:, None])
            pad = np.pad(fill, 1)
            inner = fill & pad[1:-1, :-2] & pad[1:-1, 2:] & pad[:-2, 1:-1] & pad[2:, 1:-1]
            axes[inner] = FILL[view["slot_colour"][w] % 10]
            axes[fill & ~inner] = INNER
            axes[in_slot & (np.abs(dx) <= view["line_half"]) & (rows >= m[5]) & (rows <= m[4])] = INNER
            axes[in_slot & (np.abs(dx) <= view["box_half"]) & (rows >= m[3]) & (rows <= m[2])] = INNER
            dy = rows.astype(np.int64) - int(m[1])
            axes[in_slot & (dx.astype(np.int64) ** 2 + dy ** 2 <= view["dot_r2"])] = WHITE
        else:
            axes[in_slot & (np.abs(dx) <= sw * 95 // 200) & (np.abs(rows - int(m[6])) <= view["line_half"])] = INNER
    if ax_x >= 1:
        rgb[ax_y:min(ax_y + ax_h + 1, H), ax_x - 1] = BLACK
    if ax_y + ax_h < H:
        rgb[ax_y + ax_h, max(ax_x - 1, 0):ax_x + ax_w] = BLACK
    return rgb


def paint_violins(sums, dens, view):
    return paint(*profile(sums, dens, view), view)
