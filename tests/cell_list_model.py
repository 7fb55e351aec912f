"""NumPy float32 statement of the batch link's candidate lists (csrc/batch_link.h: k_bgrid, bl_cell_list) and of the block
k_bgrid leaves per frame -- the same operations in the same order, every intermediate a float32 (no fused multiply-add: the
library is built with -ffp-contract=off; sqrt and the division are correctly rounded on both sides).

    bin_frame(xy)                 the grid of a frame and its counting sort (x0, y0, cell, inv, G, start, order)
    rect_list(grid, xy, cx, cy, rect)   the candidates of a rectangle inside cell (cx, cy): (kept positions, gathered count)
    cell_rect / quad_rect         the rectangle of a cell / of one of its four quadrants, grown by e
    frame_lists(grid, xy)         the lists as the block holds them: (list16 [cells][8] u16, overflow [entries][4][8] u16)
    lane_cell(grid, px, py)       what bl_search decides for a prediction: (cx, cy, quadrant), cx / cy may lie outside
    block layout                  grid_n, start_dwords, mp, list_off, ovf_off, grid_dwords -- the header's arithmetic

`xy` handed to rect_list / frame_lists is the frame's centres IN CELL ORDER, float32 (m, 2).  Within a cell the order of
the device's counting sort is whatever its LDS atomics made it, so a test of the device's lists passes the centres it read
back from the block; bin_frame's own order is by detection number within a cell.
"""
import numpy as np

F = np.float32
BL_LIST, BG_CAND, BL_OVF = 8, 32, 8
FLAG, SPLIT = 0xFFFF, 0xFFFE


def grid_n(m):
    return 16 if m <= 128 else (32 if m <= 600 else (48 if m <= 1300 else 64))


def has_lists(m):
    return grid_n(m) <= 32


def start_dwords(G):
    return ((G * G + 2) // 2 + 3) // 4 * 4


def mp(m):
    return (m + 1 + 7) // 8 * 8


def list_off(m):
    return 16 + start_dwords(grid_n(m)) + 2 * mp(m) + mp(m) // 2


def ovf_off(m):
    G = grid_n(m)
    return list_off(m) + G * G * BL_LIST // 2


def grid_dwords(m):
    raw = ovf_off(m) + BL_OVF * 4 * BL_LIST // 2 if has_lists(m) else list_off(m)
    return (raw + 255) // 256 * 256


class Grid:
    def __init__(self, x0, y0, cell, inv, G, m, start):
        self.x0, self.y0, self.cell, self.inv, self.G, self.m, self.start = x0, y0, cell, inv, G, m, start


def bin_frame(xy):
    """(Grid, order): order[k] = the detection at position k of the cell-ordered list (ascending within a cell)."""
    xy = np.asarray(xy, F).reshape(-1, 2)
    m = len(xy)
    G = grid_n(m)
    if m:
        lo_x, hi_x, lo_y, hi_y = xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()
    else:
        lo_x = lo_y = F(0); hi_x = hi_y = F(1)
    extent = max(max(F(hi_x - lo_x), F(hi_y - lo_y)), F(1))
    cell = F(extent / F(G - 2))
    inv = F(F(1) / cell)
    x0, y0 = F(lo_x - cell), F(lo_y - cell)
    cx = np.clip(np.floor((xy[:, 0] - x0) * inv).astype(np.int64), 0, G - 1)
    cy = np.clip(np.floor((xy[:, 1] - y0) * inv).astype(np.int64), 0, G - 1)
    c = cy * G + cx
    order = np.argsort(c, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=G * G))]).astype(np.int64)
    return Grid(x0, y0, cell, inv, G, m, start), order


def grow(g):
    return F(F(4e-3) + F(2e-4) * g.cell)


def cell_rect(g, cx, cy):
    e = grow(g)
    return (F(g.x0 + F(cx) * g.cell) - e, F(g.x0 + F(cx + 1) * g.cell) + e,
            F(g.y0 + F(cy) * g.cell) - e, F(g.y0 + F(cy + 1) * g.cell) + e)


def quad_rect(g, cx, cy, q):
    """Quadrant q = qx + 2 qy of cell (cx, cy): half a cell wide, the same e (batch_link.h: bl_quad_rect)."""
    e = grow(g)
    hx, hy = F(cx) + F(0.5) * F(q & 1), F(cy) + F(0.5) * F(q >> 1)
    return (F(g.x0 + hx * g.cell) - e, F(g.x0 + F(hx + F(0.5)) * g.cell) + e,
            F(g.y0 + hy * g.cell) - e, F(g.y0 + F(hy + F(0.5)) * g.cell) + e)


def rect_list(g, xy, cx, cy, rect):
    """bl_rect_list: (positions kept by the pruning, all of them, ascending; candidates gathered).  The device flags the
    rectangle when more than BG_CAND were gathered (the pruning is then skipped: kept is None) or more than BL_LIST kept."""
    ax, bx, ay, by = rect
    G, start = g.G, g.start
    x, y = xy[:, 0], xy[:, 1]
    u2, ju = F(3.0e38), 0

    def far2(a, b):
        nonlocal u2, ju
        if b <= a:
            return
        dx = np.maximum(np.abs(x[a:b] - ax), np.abs(x[a:b] - bx))
        dy = np.maximum(np.abs(y[a:b] - ay), np.abs(y[a:b] - by))
        v = dx * dx + dy * dy
        k = int(np.argmin(v))
        if v[k] < u2:
            u2, ju = v[k], a + k

    for r in range(G):
        xl, xh = max(cx - r, 0), min(cx + r, G - 1)
        for yy in range(max(cy - r, 0), min(cy + r, G - 1) + 1):
            if yy == cy - r or yy == cy + r:
                far2(start[yy * G + xl], start[yy * G + xh + 1])
            else:
                if cx - r >= 0:
                    far2(start[yy * G + cx - r], start[yy * G + cx - r + 1])
                if cx + r < G:
                    far2(start[yy * G + cx + r], start[yy * G + cx + r + 1])
        reach = F(F(r + 1) * g.cell)
        if u2 <= F(reach * reach):
            break
    e = grow(g)
    T = F(F(np.sqrt(u2)) * F(1.0001)) + F(1.0)
    T2 = F(T * T)
    rho = min(int(F(F(T + e) * g.inv)) + 2, G)
    cand = []
    zero = F(0)
    for yy in range(max(cy - rho, 0), min(cy + rho, G - 1) + 1):
        a, b = start[yy * G + max(cx - rho, 0)], start[yy * G + min(cx + rho, G - 1) + 1]
        if b <= a:
            continue
        dx = np.maximum(np.maximum(ax - x[a:b], x[a:b] - bx), zero)
        dy = np.maximum(np.maximum(ay - y[a:b], y[a:b] - by), zero)
        cand.extend((a + np.flatnonzero(dx * dx + dy * dy <= T2)).tolist())
    n = len(cand)
    if n > BG_CAND:
        return None, n
    eps, beta = F(1.00003), F(0.6)
    cj = np.array(cand, np.int64)
    xa, xb, ya, yb = ax - x[cj], bx - x[cj], ay - y[cj], by - y[cj]
    s = np.stack([xa * xa + ya * ya, xb * xb + ya * ya, xa * xa + yb * yb, xb * xb + yb * yb])     # [corner][candidate]
    lim = s * eps + beta
    ua, ub, va, vb = F(ax - x[ju]), F(bx - x[ju]), F(ay - y[ju]), F(by - y[ju])
    ulim = np.array([F(ua * ua + va * va) * eps + beta, F(ub * ub + va * va) * eps + beta,
                     F(ua * ua + vb * vb) * eps + beta, F(ub * ub + vb * vb) * eps + beta], F)
    kept = []
    for i in range(n):
        beaten = cand[i] != ju and bool(np.all(s[:, i] > ulim))
        if not beaten:
            over = np.all(s[:, i:i + 1] > lim, axis=0)
            over[i] = False
            beaten = bool(over.any())
        if not beaten:
            kept.append(cand[i])
    return kept, n


def flagged(kept):
    return kept is None or len(kept) > BL_LIST


def _row(kept, m):
    return [FLAG] * BL_LIST if flagged(kept) else kept + [m] * (BL_LIST - len(kept))


def frame_lists(g, xy, ovf=BL_OVF, detail=None):
    """(list16 [cells][BL_LIST], overflow [ovf][4][BL_LIST]) as the block holds them.  A flagged slot: FLAG in the first
    u16, the rest is unspecified (masked to FLAG here); a split cell: SPLIT, its entry, the rest unspecified (zeros here).  Unused overflow
    entries are zero.  detail: a dict that receives, per crowded cell, (kept or None, gathered, the four quadrants' kept)."""
    G, m = g.G, g.m
    xy = np.asarray(xy, F).reshape(-1, 2)
    lists = np.zeros((G * G, BL_LIST), np.uint16)
    over = np.zeros((ovf, 4, BL_LIST), np.uint16)
    crowded = []
    for c in range(G * G):
        kept, n = rect_list(g, xy, c % G, c // G, cell_rect(g, c % G, c // G))
        lists[c] = _row(kept, m)
        if flagged(kept):
            crowded.append((c, kept, n))
    for k, (c, kept, n) in enumerate(crowded):
        quads = [rect_list(g, xy, c % G, c // G, quad_rect(g, c % G, c // G, q))[0] for q in range(4)] if k < ovf or detail is not None else None
        if detail is not None:
            detail[c] = (kept, n, quads)
        if k >= ovf:
            continue
        for q in range(4):
            over[k, q] = _row(quads[q], m)
        if not any(flagged(qk) for qk in quads):
            lists[c] = [SPLIT, k] + [0] * (BL_LIST - 2)
    return lists, over


def lane_cell(g, px, py):
    """bl_search's decision for a prediction (float64 in): (cx, cy, q); cx / cy outside [0, G) mean outside the grid."""
    ux = F(F(F(px) - g.x0) * g.inv)
    uy = F(F(F(py) - g.y0) * g.inv)
    fx, fy = np.floor(ux), np.floor(uy)
    q = int(F(ux - fx) >= F(0.5)) + 2 * int(F(uy - fy) >= F(0.5))
    return int(fx), int(fy), q
