"""NumPy statement of the figures' rendering rules ("The figures"): what csrc/plots.hip must produce byte
for byte.  The painter is sequential -- start dots, then track by track in rank order, later over earlier --;
``key_canvas_max`` is the same canvas as "the largest key wins", which is how the device paints it."""
import numpy as np

GRID = (176, 176, 176)
BAR_FILL = (143, 187, 218)


def lut():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viridis_r_u8.npy"))


def runs(ids):
    """(start flag per row, track number per row, first row per track) of the contiguous runs of equal ids."""
    ids = np.asarray(ids)
    n = len(ids)
    flag = np.ones(n, bool)
    flag[1:] = ids[1:] != ids[:-1]
    seg = np.cumsum(flag) - 1
    return flag, seg, np.flatnonzero(flag)


def data_coordinates(ids, x, y, mode, px):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if mode == 1 and len(x):
        _, seg, first = runs(ids)
        x, y = x - x[first][seg], y - y[first][seg]
    with np.errstate(all="ignore"):
        return x / np.float64(px), y / np.float64(px)


def extent(ids, x, y, mode, px):
    u, v = data_coordinates(ids, x, y, mode, px)
    ok = np.isfinite(u) & np.isfinite(v)
    if not ok.any():
        return np.array([np.inf, -np.inf, np.inf, -np.inf])
    return np.array([u[ok].min(), u[ok].max(), v[ok].min(), v[ok].max()])


def colour_values(dist):
    """(c, LUT index, rank) per track."""
    dist = np.asarray(dist, np.float64)
    nt = len(dist)
    c = np.zeros(nt)
    if nt and np.isfinite(dist).all():
        span = dist.max() - dist.min()
        if span > 0 and np.isfinite(span):
            c = (dist - dist.min()) / span
    idx = np.minimum(255, (c * 256.0).astype(np.int64))
    rank = np.array([int(np.sum((c > c[t]) | ((c == c[t]) & (np.arange(nt) < t)))) for t in range(nt)], np.int64)
    return c, idx, rank


def disc(r2):
    rad = int(np.floor(np.sqrt(r2)))
    return [(dx, dy) for dy in range(-rad, rad + 1) for dx in range(-rad, rad + 1) if dx * dx + dy * dy <= r2]


def _centres(ids, x, y, view):
    """Per row: pixel relative to the axes' top-left corner (as float, exact integers) and whether it is drawn at all."""
    u, v = data_coordinates(ids, x, y, view["mode"], view["px"])
    ok = np.isfinite(u) & np.isfinite(v)
    with np.errstate(all="ignore"):
        fc = np.floor((u - view["u0"]) / view["upp"])
        fr = np.floor((v - view["v0"]) / view["upp"])
    # (far outside no disc reaches in; clip so that the integer conversion below is defined)
    far = 1e6
    ok &= (np.abs(fc) < far) & (np.abs(fr) < far)
    c = np.where(ok, fc, 0).astype(np.int64)
    r = view["ax_h"] - 1 - np.where(ok, fr, 0).astype(np.int64)
    return c, r, ok


def key_canvas_sequential(ids, x, y, dist, view):
    """The painter: key 1 around every track's first row (mode 0), then the tracks in rank order, a row at a time."""
    keys = np.zeros((view["H"], view["W"]), np.uint32)
    if len(ids) == 0 or len(dist) == 0:
        return keys
    flag, seg, first = runs(ids)
    c, r, ok = _centres(ids, x, y, view)
    _, _, rank = colour_values(dist)

    def dot(i, r2, key):
        for dx, dy in disc(r2):
            pc, pr = c[i] + dx, r[i] + dy
            if 0 <= pc < view["ax_w"] and 0 <= pr < view["ax_h"]:
                keys[view["ax_y"] + pr, view["ax_x"] + pc] = key

    nt = len(dist)
    if view["mode"] == 0:
        for i in first:
            if ok[i] and seg[i] < nt:
                dot(i, view["r2_start"], 1)
    for t in np.argsort(rank, kind="stable"):
        for i in np.flatnonzero(seg == t):
            if ok[i]:
                dot(i, view["r2_dot"], 2 + rank[t])
    return keys


def key_canvas_max(ids, x, y, dist, view):
    """The same canvas: every pixel holds the largest key painted on it."""
    keys = np.zeros((view["H"], view["W"]), np.uint32)
    if len(ids) == 0 or len(dist) == 0:
        return keys
    flag, seg, first = runs(ids)
    c, r, ok = _centres(ids, x, y, view)
    _, _, rank = colour_values(dist)
    ok = ok & (seg < len(dist))
    row_key = (2 + rank[np.minimum(seg, len(dist) - 1)]).astype(np.uint32)
    flat = keys.reshape(-1)

    def dots(sel, r2, key):
        for dx, dy in disc(r2):
            pc, pr = c[sel] + dx, r[sel] + dy
            inside = (pc >= 0) & (pc < view["ax_w"]) & (pr >= 0) & (pr < view["ax_h"])
            at = (view["ax_y"] + pr[inside]) * view["W"] + view["ax_x"] + pc[inside]
            np.maximum.at(flat, at, key[inside] if isinstance(key, np.ndarray) else np.uint32(key))

    if view["mode"] == 0:
        dots(np.flatnonzero(flag & ok), view["r2_start"], 1)
    sel = np.flatnonzero(ok)
    dots(sel, view["r2_dot"], row_key[sel])
    return keys


def compose(keys, dist, view):
    """Key canvas -> RGB: white, the axes' frame, grid, start dots and tracks, then the colour bar and its frame."""
    table = lut()
    H, W = view["H"], view["W"]
    rgb = np.full((H, W, 3), 255, np.uint8)
    x0, y0, w, h = view["ax_x"], view["ax_y"], view["ax_w"], view["ax_h"]
    rgb[max(y0 - 1, 0):y0 + h + 1, max(x0 - 1, 0):x0 + w + 1] = 0
    inner = rgb[y0:y0 + h, x0:x0 + w]
    inner[:] = 255
    for col in view["grid_cols"]:
        if x0 <= col < x0 + w:
            inner[:, col - x0] = GRID
    for row in view["grid_rows"]:
        if y0 <= row < y0 + h:
            inner[row - y0, :] = GRID
    k = keys[y0:y0 + h, x0:x0 + w]
    inner[k == 1] = 0
    if len(dist):
        _, idx, rank = colour_values(dist)
        idx_of_rank = np.zeros(len(dist), np.int64)
        idx_of_rank[rank] = idx
        on = k >= 2
        inner[on] = table[idx_of_rank[k[on].astype(np.int64) - 2]]
    if view["bar_w"] > 0:
        bx, by, bw, bh = view["bar_x"], view["bar_y"], view["bar_w"], view["bar_h"]
        rgb[max(by - 1, 0):by + bh + 1, max(bx - 1, 0):bx + bw + 1] = 0
        j = np.arange(bh)
        rgb[by:by + bh, bx:bx + bw] = table[np.minimum(255, ((bh - 1 - j) * 256) // bh)][:, None, :]
    return rgb


def paint_tracks(ids, x, y, dist, view, sequential=False):
    keys = (key_canvas_sequential if sequential else key_canvas_max)(ids, x, y, dist, view)
    return compose(keys, dist, view)


def make_view(mode, W, H, ax, u0, v0, upp, px=1.0, r2_dot=1, r2_start=4, grid_cols=(), grid_rows=(), bar=(0, 0, 0, 0)):
    return {"mode": mode, "W": W, "H": H, "ax_x": ax[0], "ax_y": ax[1], "ax_w": ax[2], "ax_h": ax[3], "u0": float(u0),
            "v0": float(v0), "upp": float(upp), "px": float(px), "r2_dot": r2_dot, "r2_start": r2_start,
            "grid_cols": list(grid_cols), "grid_rows": list(grid_rows), "bar_x": bar[0], "bar_y": bar[1], "bar_w": bar[2],
            "bar_h": bar[3]}


def to_struct(view):
    """The model's view as ``ysmr_plot_view``."""
    from ysmr_amd import _lib
    v = _lib.PlotView()
    v.px, v.u0, v.v0, v.units_per_pixel = view["px"], view["u0"], view["v0"], view["upp"]
    v.mode, v.width, v.height = view["mode"], view["W"], view["H"]
    v.ax_x, v.ax_y, v.ax_w, v.ax_h = view["ax_x"], view["ax_y"], view["ax_w"], view["ax_h"]
    v.r2_dot, v.r2_start = view["r2_dot"], view["r2_start"]
    v.n_grid_cols, v.n_grid_rows = len(view["grid_cols"]), len(view["grid_rows"])
    for k, c in enumerate(view["grid_cols"]):
        v.grid_cols[k] = c
    for k, r in enumerate(view["grid_rows"]):
        v.grid_rows[k] = r
    v.bar_x, v.bar_y, v.bar_w, v.bar_h = view["bar_x"], view["bar_y"], view["bar_w"], view["bar_h"]
    return v


# ---- the angle histogram ---------------------------------------------------------------------------------------------

def headings(ids, x, y, moving, lag, arctan2=np.arctan2):
    """(selected rows as a mask, heading per row -- NaN where there is none).  ``arctan2``: NumPy's, or a model of it
    (atan2_exact.atan2_cr)."""
    ids, x, y, moving = np.asarray(ids), np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(moving)
    n = len(ids)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0)
    flag, seg, first = runs(ids)
    rows = np.bincount(seg)
    ones = np.bincount(seg, weights=(moving == 1)).astype(np.int64)
    passes = ones.astype(np.float64) / rows.astype(np.float64) > 0.7
    selected = passes[seg] & (moving == 1)
    h = np.full(n, np.nan)
    i = np.arange(n)
    has = i - lag >= first[seg]
    j = i[has]
    with np.errstate(all="ignore"):
        h[j] = arctan2(x[j] - x[j - lag], y[j] - y[j - lag])
    return selected, h


def angle_histogram(ids, x, y, moving, lag, edges, arctan2=np.arctan2):
    selected, h = headings(ids, x, y, moving, lag, arctan2)
    hs = h[selected]
    counts, _ = np.histogram(hs[~np.isnan(hs)], edges)
    return counts.astype(np.int64), int(selected.sum())


def edge_clearance(ids, x, y, moving, lag, edges, exact=()):
    """Smallest distance of a selected row's heading to an edge, the headings listed in ``exact`` left out."""
    selected, h = headings(ids, x, y, moving, lag)
    hs = h[selected]
    hs = hs[~np.isnan(hs)]
    for e in exact:
        hs = hs[hs != e]
    if len(hs) == 0:
        return np.inf
    return float(np.abs(hs[:, None] - np.asarray(edges)[None, :]).min())


# ---- the wedges ------------------------------------------------------------------------------------------------------

def wedge_directions(edges):
    """(east, north) of every boundary heading (clockwise from north); the last repeats the first."""
    d = np.stack([np.sin(edges), np.cos(edges)], axis=1)
    d[-1] = d[0]
    return np.ascontiguousarray(d)


def _wedge_fill(pe, pn, dirs, r2):
    """Wedge number where the pixel is filled, else -1 (arrays of int64)."""
    n_bins = len(r2)
    e, nn = pe.astype(np.float64), pn.astype(np.float64)
    d2 = pe * pe + pn * pn
    out = np.full(pe.shape, -1, np.int64)
    found = d2 == 0
    prev = dirs[0, 0] * nn - dirs[0, 1] * e
    for k in range(n_bins):
        nxt = dirs[k + 1, 0] * nn - dirs[k + 1, 1] * e
        here = ~found & (prev <= 0) & (nxt > 0)
        out[here & (d2 <= r2[k])] = k
        found |= here
        prev = nxt
    return out


def wedges(W, H, cx, cy, dirs, r2, ring_r2):
    r2 = np.asarray(r2, np.int64)
    row, col = np.mgrid[0:H, 0:W].astype(np.int64)
    pe, pn = col - cx, cy - row
    rgb = np.full((H, W, 3), 255, np.uint8)
    d2 = pe * pe + pn * pn
    beyond = lambda a, b: a * a + b * b > ring_r2                                # noqa: E731
    ring = (d2 <= ring_r2) & (beyond(pe - 1, pn) | beyond(pe + 1, pn) | beyond(pe, pn - 1) | beyond(pe, pn + 1))
    rgb[ring] = GRID
    k = _wedge_fill(pe, pn, dirs, r2)
    inner = np.ones((H, W), bool)
    for de, dn in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        inner &= _wedge_fill(pe + de, pn + dn, dirs, r2) == k
    rgb[(k >= 0) & inner] = BAR_FILL
    rgb[(k >= 0) & ~inner] = 0
    return rgb
