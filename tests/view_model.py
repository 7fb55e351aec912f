"""The sequential painter of the detection view, in numpy -- test helper, not collected.

A frame is expanded to B, G, R; then every detection's outline (``luminosity_model.int_corners`` + ``line8``, corner i-1 ->
corner i, pixels outside the frame dropped) in (255, 0, 0); then every row's id and dot (``annotate_model.paint_frame``,
style 0) in (0, 255, 0).  ``pack_dib`` of annotate_model stores the result.

``line8_window`` gives the pixels of ``line8`` that lie inside a frame without walking the line -- for the boxes whose
corners sit a million pixels away, where the list ``line8`` returns would take a quarter of a gigabyte per edge.  It is the
same recurrence summed up (after i major steps the minor coordinate has moved floor((2 d_minor i + d_major - 1) /
(2 d_major)) times), and tests/test_view_cpu.py pins it to ``line8`` itself on random segments before it is relied on.

``cases()`` is the table of edge cases shared by the CPU, the GPU and the stand-alone host test.
"""
import math

import numpy as np

import annotate_model as A
import luminosity_model as M

ROW_DTYPE = np.dtype([("frame", "<i4"), ("track_id", "<i4"), ("x", "<f8"), ("y", "<f8"),
                      ("w", "<f4"), ("h", "<f4"), ("angle", "<f4"), ("disappeared", "<i4")])
BOX_COLOUR = (255, 0, 0)
FAR = 4096          # a segment with an end this far from the origin is not walked


def line8_window(p, q, H, W):
    """The pixels of ``line8(p, q)`` inside [0, W) x [0, H), as a set."""
    (x0, y0), (x1, y1) = p, q
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, abs(y1 - y0)
    sy = 1 if y1 >= y0 else -1
    if dy > dx:          # one pixel per row: the rows of the frame that the line crosses
        ys = np.arange(H, dtype=np.int64)
        k = (ys - y0) * sy
        ok = (k >= 0) & (k <= dy)
        xs = x0 + (2 * dx * k + dy - 1) // (2 * dy)
        ok &= (xs >= 0) & (xs < W)
        return {(int(x), int(y)) for x, y in zip(xs[ok], ys[ok])}
    xs = np.arange(max(x0, 0), min(x1, W - 1) + 1, dtype=np.int64)       # one pixel per column
    i = xs - x0
    ys = y0 + sy * ((2 * dy * i + dx - 1) // (2 * dx)) if dx else np.full(len(xs), y0, np.int64)
    ok = (ys >= 0) & (ys < H)
    return {(int(x), int(y)) for x, y in zip(xs[ok], ys[ok])}


def outline(pts, H, W):
    """Set of (x, y) inside the frame that the closed outline of the four corners paints."""
    px = set()
    for i in range(len(pts)):
        p, q = tuple(pts[i - 1]), tuple(pts[i])
        if max(abs(v) for v in p + q) > FAR:
            px |= line8_window(p, q, H, W)
        else:
            px |= {(x, y) for (x, y) in M.line8(p, q) if 0 <= x < W and 0 <= y < H}
    return px


def marks_of_rows(rows, frame):
    """annotate_model marks (style 0) of the rows of one frame: (int(x), int(y)), the id as uint32; rows whose position is
    not finite are left out."""
    sel = rows[(rows["frame"] == frame) & np.isfinite(rows["x"]) & np.isfinite(rows["y"])]
    marks = np.zeros(len(sel), A.MARK_DTYPE)
    lim = np.iinfo(np.int32)
    marks["x"] = np.clip(np.trunc(sel["x"]), lim.min, lim.max).astype(np.int32)
    marks["y"] = np.clip(np.trunc(sel["y"]), lim.min, lim.max).astype(np.int32)
    marks["track_id"] = sel["track_id"].astype(np.int64) & 0xFFFFFFFF
    return marks


def paint(frames, det, det_count, rows, first_frame_index):
    """frames u8 [n, H, W(, 3)], det f32 [n, max_det, 5], det_count i32 [n], rows ROW_DTYPE (any order, any frames) ->
    the painted frames u8 [n, H, W, 3]."""
    out = A.to_bgr(frames)
    n, H, W = out.shape[:3]
    for f in range(n):
        for d in range(min(max(int(det_count[f]), 0), det.shape[1])):
            for (x, y) in outline(M.int_corners(det[f, d]), H, W):
                out[f, y, x] = BOX_COLOUR
        A.paint_frame(out[f], marks_of_rows(rows, first_frame_index + f))
    return out


def row(frame, track_id, x, y, w=3.0, h=2.0, angle=0.0, disappeared=0):
    return (frame, np.uint32(track_id).astype(np.int32), x, y, w, h, angle, disappeared)


H, W, N = 37, 50, 3
CLAMP = float(1 << 20)


def cases(first=0):
    """(det f32 [3, max_det, 5], det_count i32 [3], rows ROW_DTYPE) for frames of 37 x 50.  Frame 0: the boxes; frame 1: the
    marks (and a box under one of them); frame 2: nothing at all."""
    boxes0 = [
        (12.0, 9.0, 9.0, 5.0, 0.0), (30.5, 8.5, 7.0, 4.0, 90.0), (40.0, 20.0, 6.0, 3.0, -90.0),       # angles 0, 90, -90
        (20.3, 20.6, 13.0, 6.0, 33.0), (33.1, 29.4, 10.5, 4.2, -71.5), (9.9, 27.2, 8.0, 8.0, 45.0),    # oblique
        (25.0, 14.0, 0.0, 0.0, 0.0), (44.0, 33.0, 5.0, 0.0, 0.0), (4.0, 18.0, 6.0, 0.0, 27.0),         # (0, 0) and (w, 0) boxes
        (1.0, 12.0, 8.0, 5.0, 15.0), (48.5, 25.0, 9.0, 4.0, -20.0), (22.0, 0.5, 6.0, 7.0, 10.0),       # straddling the left, right, top
        (27.0, 36.0, 7.0, 6.0, 80.0), (0.0, 0.0, 7.0, 7.0, 30.0), (49.0, 36.0, 9.0, 5.0, 60.0),        # ... bottom edge, two corners
        (-30.0, -20.0, 9.0, 5.0, 12.0), (80.0, 18.0, 6.0, 6.0, 0.0),                                  # wholly outside
        (25.0, 18.0, 4.0e6, 4.0e6, 0.0),             # all four corners at the +-2^20 clamp: the frame lies inside, untouched
        (25.0, 18.0, 4.0e6, 4.0e6, 45.0),            # ... turned: corners clamped on one axis each
        (CLAMP, 18.0, 2.0 * CLAMP, 9.0, 0.0),        # a box from inside the frame to the clamp: two horizontal edges cross it
        (12.0, -CLAMP / 2, 5.0, CLAMP + 40.0, 1.0e-3),   # a very long, slightly tilted box entering from the top
        (25.0 + 3.6e5 * math.cos(math.radians(33.7)), 18.0 + 3.6e5 * math.sin(math.radians(33.7)), 7.3e5, 11.0, 33.7),
        # ^ a long oblique sliver from far away whose x-major edges pass through the frame
    ]
    boxes1 = [(24.0, 12.0, 30.0, 8.0, 0.0),          # the id of the mark at (30, 24) crosses this box's lower edge: green wins
              (30.0, 24.0, 3.0, 3.0, 0.0)]
    max_det = len(boxes0) + 3
    det = np.zeros((N, max_det, 5), np.float32)
    det[:] = (5.0, 5.0, 40.0, 40.0, 17.0)            # what lies behind det_count must not be painted
    det[0, :len(boxes0)] = boxes0
    det[1, :len(boxes1)] = boxes1
    det_count = np.array([len(boxes0), len(boxes1), 0], np.int32)
    f1 = first + 1
    rows = np.array([
        row(f1, 7, 30.9, 24.9), row(f1, 42, 12.2, 30.0), row(f1, 123, 44.0, 20.5), row(f1, 4567, 20.0, 10.0),
        row(f1, 89012, 25.5, 35.99),                              # ids of 1 to 5 digits
        row(f1, 4294967295, 8.0, 18.0), row(f1, 3000000000, 2.0, 36.0),     # ten digits (ids are uint32)
        row(f1, 5, 17.0, 22.0, 0.0, 0.0, 0.0, 3),                 # a disappeared row
        row(f1, 6, -0.9, -0.9), row(f1, 8, 49.999, 0.5), row(f1, 9, 55.0, 40.0), row(f1, 10, -3.0e9, 5.0e9),
        row(f1, 11, float("nan"), 3.0), row(f1, 12, 3.0, float("inf")),
        row(first + 0, 31, 25.0, 18.0),                           # frame 0: a mark over the boxes
        row(first - 1, 1, 10.0, 10.0), row(first + N, 2, 10.0, 10.0), row(first + 1000, 3, 10.0, 10.0),   # outside the batch
    ], ROW_DTYPE)
    return det, det_count, rows


def frames_of(channels, seed=5):
    rng = np.random.default_rng(seed)
    shape = (N, H, W) if channels == 1 else (N, H, W, 3)
    return rng.integers(0, 200, shape, dtype=np.uint8)      # (below 255: a painted pixel is never the frame's own value)
