"""NumPy restatement of the luminosity mode of the reference's frame loop -- test helper, not collected.

What it restates (paths under the reference tree):

* ``box_points`` / ``int_corners``  ``np.intp(cv2.boxPoints(rect))``                 ysmr/track_eval.py:293
* ``line8`` / ``fill``              ``cv2.fillPoly(mask, [box], 255)``               ysmr/track_eval.py:295
                                    (8-connected LineIterator + the 16.16 edge-table scanline fill of OpenCV's drawing.cpp)
* ``masked_mean`` / ``luminosity``  ``cv2.mean(gray, mask)[0] / 100``                ysmr/track_eval.py:296-300
* ``bgr2gray``                      ``cv2.cvtColor(frame, COLOR_BGR2GRAY)``          ysmr/track_eval.py:180
* ``Linker``                        ``CentroidTracker.update`` without GSFF, points of any dimension  ysmr/tracker.py:93-230

The cv2 half is an upstream recollection and PARITY-UNPINNED (cv2 is importable neither where this suite is built nor
where it runs; tests/test_luminosity_cpu.py cross-checks it against cv2 wherever cv2 is present, and against an independent
geometric formulation everywhere).  The linker is pinned: it reproduces tests/golden/tracker_lum_*.npz, which the
reference's own tracker.py wrote.

The fill is kept set-based on purpose -- it is what the device kernel's run-per-row arithmetic is judged by.
"""
import math

import numpy as np

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT


def box_points(cx, cy, w, h, ang):
    """cv2.boxPoints: float32 arithmetic, cos / sin evaluated in double and rounded to float32."""
    f = np.float32
    a_ = float(f(ang)) * math.pi / 180.0
    b = f(math.cos(a_)) * f(0.5)
    a = f(math.sin(a_)) * f(0.5)
    cx, cy, w, h = f(cx), f(cy), f(w), f(h)
    p0 = (cx - a * h - b * w, cy + b * h - a * w)
    p1 = (cx + a * h - b * w, cy - b * h - a * w)
    p2 = (f(2) * cx - p0[0], f(2) * cy - p0[1])
    p3 = (f(2) * cx - p1[0], f(2) * cy - p1[1])
    return np.array([p0, p1, p2, p3], np.float32)


def int_corners(det):
    """np.intp(boxPoints(rect)) of one detection row (cx, cy, w, h, angle): [(x, y)] * 4, truncated toward zero."""
    q = np.trunc(box_points(*[float(v) for v in det[:5]])).astype(np.int64)
    return [(int(p[0]), int(p[1])) for p in q]


def line8(p, q):
    """The pixels of LineIterator(p, q, connectivity 8, leftToRight=True)."""
    (x0, y0), (x1, y1) = p, q
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, abs(y1 - y0)
    sy = 1 if y1 >= y0 else -1
    pts = []
    x, y = x0, y0
    if dy > dx:
        err = dy - 2 * dx
        for _ in range(dy + 1):
            pts.append((x, y))
            m = err < 0
            err += -2 * dx + (2 * dy if m else 0)
            y += sy
            x += 1 if m else 0
    else:
        err = dx - 2 * dy
        for _ in range(dx + 1):
            pts.append((x, y))
            m = err < 0
            err += -2 * dy + (2 * dx if m else 0)
            x += 1
            y += sy if m else 0
    return pts


def fill(pts, H, W):
    """Set of (x, y) that cv2.fillPoly(zeros((H, W)), [pts], 255) sets: the edges as lines plus the scanline spans."""
    px = set()
    n = len(pts)
    edges = []
    for i in range(n):
        p, q = pts[i - 1], pts[i]
        for (x, y) in line8(tuple(p), tuple(q)):
            if 0 <= x < W and 0 <= y < H:
                px.add((x, y))
        if p[1] == q[1]:
            continue
        if p[1] > q[1]:
            p, q = q, p
        X0, X1 = int(p[0]) << XY_SHIFT, int(q[0]) << XY_SHIFT
        d = X1 - X0
        dy = int(q[1] - p[1])
        dxs = abs(d) // dy * (1 if d >= 0 else -1)      # C division truncates
        edges.append((int(p[1]), int(q[1]), X0, dxs))
    if edges:
        for y in range(max(min(e[0] for e in edges), 0), min(max(e[1] for e in edges), H)):
            xs = sorted(e[2] + (y - e[0]) * e[3] for e in edges if e[0] <= y < e[1])
            for k in range(0, len(xs) - 1, 2):
                x1 = (xs[k] + XY_ONE - 1) >> XY_SHIFT
                x2 = xs[k + 1] >> XY_SHIFT
                for x in range(max(x1, 0), min(x2, W - 1) + 1):
                    px.add((x, y))
    return px


def bgr2gray(frame, gray_3x=False):
    """cv2.cvtColor(BGR2GRAY) on u8 [H][W][3]: 15-bit coefficients (OpenCV 4.x) or 14-bit (3.x)."""
    f = frame.astype(np.uint32)
    if gray_3x:
        return ((f[..., 0] * 1868 + f[..., 1] * 9617 + f[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)
    return ((f[..., 0] * 3735 + f[..., 1] * 19235 + f[..., 2] * 9798 + 16384) >> 15).astype(np.uint8)


def masked_mean(total, count):
    """cv2.mean(gray, mask)[0]: sum * (1.0 / count) in double, 0.0 for an empty mask."""
    return float(total) * (1.0 / float(count)) if count else 0.0


def luminosity(gray, det):
    """One detection on one gray frame -> (corners, sum, count, lum) with lum = mean / 100."""
    H, W = gray.shape
    pts = int_corners(det)
    px = fill(pts, H, W)
    total = sum(int(gray[y, x]) for (x, y) in px)
    return pts, total, len(px), masked_mean(total, len(px)) / 100


def luminosity_frame(gray, dets):
    """All detections of a frame: corners i32 [n][4][2], sum u32 [n], count u32 [n], lum f64 [n]."""
    n = len(dets)
    corners = np.zeros((n, 4, 2), np.int32)
    total = np.zeros(n, np.uint32)
    count = np.zeros(n, np.uint32)
    lum = np.zeros(n, np.float64)
    for i, d in enumerate(dets):
        c, s, k, l = luminosity(gray, d)
        corners[i], total[i], count[i], lum[i] = c, s, k, l
    return corners, total, count, lum


# ---- independent geometric formulation (the fill is judged by it in tests/test_luminosity_cpu.py) -------------------------

def inside_strict(pts, x, y):
    """Exact integer test: (x, y) strictly inside the convex quadrilateral, either orientation."""
    s = []
    for i in range(4):
        (ax, ay), (bx, by) = pts[i - 1], pts[i]
        s.append((bx - ax) * (y - ay) - (by - ay) * (x - ax))
    return all(v > 0 for v in s) or all(v < 0 for v in s)


def dist2_to_quad(pts, x, y):
    """Squared distance of (x, y) to the closed quadrilateral (0 inside)."""
    if inside_strict(pts, x, y):
        return 0.0
    best = 1e30
    for i in range(4):
        ax, ay = pts[i - 1]
        bx, by = pts[i]
        ux, uy = bx - ax, by - ay
        uu = ux * ux + uy * uy
        t = 0.0 if uu == 0 else min(1.0, max(0.0, ((x - ax) * ux + (y - ay) * uy) / uu))
        ex, ey = ax + t * ux - x, ay + t * uy - y
        best = min(best, ex * ex + ey * ey)
    return best


# ---- the linker ----------------------------------------------------------------------------------------------------------

def cdist(a, b):
    """scipy.spatial.distance.cdist(a, b) (euclidean): squares summed in coordinate order, no contraction."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    acc = np.zeros((len(a), len(b)), np.float64)
    for k in range(a.shape[1]):
        d = a[:, k][:, None] - b[:, k][None, :]
        acc = acc + d * d
    return np.sqrt(acc)


class Linker:
    """CentroidTracker(use_gsff=False).update for points of any dimension: ids, claims, disappeared counters, births in
    CPython set order, the additional_info bookkeeping (zeros for an aged track).  ``update(points, infos)`` returns
    (claimed column per track before the update or -1, columns born in id order).

    ``min_gap``: how close the run came to a decision the reference leaves to an unstable argsort or to argmin's tie rule
    -- the smallest difference between a row's two lowest distances, and between the minima of two rows that propose the
    same column."""

    def __init__(self, max_disappeared):
        self.max_disappeared = max_disappeared
        self.next_id = 0
        self.objects = {}        # id -> point (np.float64 [d]); insertion order = id order
        self.disappeared = {}
        self.info = {}
        self.min_gap = math.inf

    def _register(self, p, info):
        self.objects[self.next_id] = np.array(p, np.float64)
        self.disappeared[self.next_id] = 0
        self.info[self.next_id] = info
        self.next_id += 1

    def _age(self, i):
        self.disappeared[i] += 1
        self.info[i] = [0] * len(self.info[i])
        if self.disappeared[i] > self.max_disappeared:
            del self.objects[i]
            del self.disappeared[i]
            del self.info[i]

    def update(self, points, infos=None):
        points = np.asarray(points, np.float64)
        if infos is None:
            infos = [(0.0, 0.0, 0.0)] * len(points)
        ids = list(self.objects.keys())
        claims = [-1] * len(ids)
        born = []
        if len(points) == 0:
            for i in ids:
                self._age(i)
            return claims, born
        if not ids:
            for c in range(len(points)):
                born.append(c)
                self._register(points[c], infos[c])
            return claims, born
        D = cdist(np.array([self.objects[i] for i in ids]), points)
        row_min = D.min(axis=1)
        arg = D.argmin(axis=1)
        if D.shape[1] > 1:
            part = np.partition(D, 1, axis=1)
            self.min_gap = min(self.min_gap, float((part[:, 1] - part[:, 0]).min()))
        for c in np.unique(arg):
            same = np.sort(row_min[arg == c])
            if len(same) > 1:
                self.min_gap = min(self.min_gap, float(np.diff(same).min()))
        rows = row_min.argsort()
        cols = arg[rows]
        used_rows, used_cols = set(), set()
        for (row, col) in zip(rows, cols):
            row, col = int(row), int(col)
            if row in used_rows or col in used_cols:
                continue
            i = ids[row]
            self.objects[i] = points[col].copy()
            self.info[i] = infos[col]
            self.disappeared[i] = 0
            claims[row] = col
            used_rows.add(row)
            used_cols.add(col)
        unused_rows = set(range(D.shape[0])).difference(used_rows)
        unused_cols = set(range(D.shape[1])).difference(used_cols)
        if D.shape[0] >= D.shape[1]:
            for row in unused_rows:
                self._age(ids[row])
        else:
            for col in unused_cols:          # CPython set iteration order, as upstream
                born.append(col)
                self._register(points[col], infos[col])
        return claims, born

    def rows(self, frame):
        """The rows track_bacteria appends after this update (track_eval.py:313-316): one per live track, id order --
        (frame, id, x, y, w, h, deg, disappeared)."""
        return [(frame, i, float(p[0]), float(p[1])) + tuple(float(v) for v in self.info[i]) + (self.disappeared[i],)
                for i, p in self.objects.items()]
