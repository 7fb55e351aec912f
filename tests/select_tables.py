"""Synthetic (TRACK_ID, POSITION_T)-ordered tables for the select_tracks tests: tracks with holes,
jumps, lost ('disappeared') rows, odd shapes and sizes, positions near and beyond the frame -- and the builders of the
tables at the sizes of a real video (tests/test_gpu_tables_at_scale.py): dust tracks by the million, spans beyond uint16,
rows in the tracker's emission order, rows of mixed values for the formatter."""
import numpy as np
import pandas as pd


def make_table(seed, n_tracks=60, height=400, width=600, max_len=260):
    rng = np.random.default_rng(seed)
    parts = []
    for tid in range(n_tracks):
        n = int(rng.integers(5, max_len))
        t0 = int(rng.integers(0, 200))
        frames = t0 + np.arange(n)
        keep = rng.random(n) > rng.choice([0.0, 0.0, 0.0, 0.02, 0.15])          # missing frames
        if rng.random() < 0.3 and n > 40:                             # one long gap
            g = int(rng.integers(10, n - 20))
            keep[g:g + int(rng.integers(3, 12))] = False
        keep[0] = True
        frames = frames[keep]
        n = len(frames)
        kind = rng.choice(["rod", "rod", "rod", "rod", "big", "round", "edge", "outside", "excursion"])
        cx, cy = rng.uniform(0.1, 0.9) * width, rng.uniform(0.1, 0.9) * height
        if kind == "edge":
            cx = rng.uniform(0.0, 0.05) * width
        if kind == "outside":
            cx = -3.0
        step = rng.normal(0, rng.choice([0.3, 1.0, 2.0]), (n, 2))
        jumps = rng.random(n) < rng.choice([0.0, 0.0, 0.01, 0.05])
        step[jumps] += rng.normal(0, 40, (int(jumps.sum()), 2))
        xy = np.cumsum(step, axis=0) + (cx, cy)
        if kind == "excursion":                                       # mean inside the frame, one row outside
            xy[:, 0] = np.clip(xy[:, 0], 0.06 * width, None)
            xy[n // 2, 0] = -0.5
        w = np.float32(rng.normal(6.0, 0.6, n)).astype(np.float64)
        h = np.float32(rng.normal(2.0, 0.25, n)).astype(np.float64)
        if kind == "big":
            w *= 4
            h *= 3
        if kind == "round":
            w = np.float32(rng.normal(4.2, 0.3, n)).astype(np.float64)
            h = w * np.float32(0.9)
        swap = rng.random(n) < 0.5
        w, h = np.where(swap, h, w), np.where(swap, w, h)
        lost = rng.random(n) < rng.choice([0.0, 0.0, 0.03, 0.2])
        w[lost] = 0.0
        h[lost] = 0.0
        blow = rng.random(n) < 0.02
        w[blow] *= 3.0
        deg = np.float32(rng.uniform(-90, 0, n)).astype(np.float64)
        deg[lost] = 0.0
        parts.append(pd.DataFrame({"TRACK_ID": np.full(n, tid, np.uint32), "POSITION_T": frames.astype(np.uint32),
                                   "POSITION_X": xy[:, 0], "POSITION_Y": xy[:, 1], "WIDTH": w, "HEIGHT": h,
                                   "DEGREES_ANGLE": deg}))
    return pd.concat(parts, ignore_index=True)


def _shapes_and_holes(rng, n):
    """The frames kept of a track of n rows (holes, one long gap) and its WIDTH / HEIGHT / DEGREES_ANGLE kinds and lost rows,
    as make_table draws them."""
    keep = rng.random(n) > rng.choice([0.0, 0.0, 0.0, 0.02, 0.15])
    if rng.random() < 0.3 and n > 40:
        g = int(rng.integers(10, n - 20))
        keep[g:g + int(rng.integers(3, 12))] = False
    keep[0] = True
    m = int(keep.sum())
    kind = rng.choice(["rod", "rod", "rod", "rod", "big", "round"])
    w = np.float32(rng.normal(6.0, 0.6, m)).astype(np.float64)
    h = np.float32(rng.normal(2.0, 0.25, m)).astype(np.float64)
    if kind == "big":
        w *= 4
        h *= 3
    if kind == "round":
        w = np.float32(rng.normal(4.2, 0.3, m)).astype(np.float64)
        h = w * np.float32(0.9)
    swap = rng.random(m) < 0.5
    w, h = np.where(swap, h, w), np.where(swap, w, h)
    lost = rng.random(m) < rng.choice([0.0, 0.0, 0.03, 0.2])
    w[lost] = 0.0
    h[lost] = 0.0
    deg = np.float32(rng.uniform(-90, 0, m)).astype(np.float64)
    deg[lost] = 0.0
    return keep, w, h, deg, lost


def lattice_table(seed, n_tracks=40, max_len=300, grid=0.5, height=400, width=600):
    """Tracks whose positions are multiples of `grid`, as the rows of a video tracked with 'disable gsff' are (raw
    minAreaRect centres: float32 values, mostly multiples of 0.5): a start on the lattice, then steps of -4 .. 4 grid units per
    axis and frame, about one step in ten zero (a lost track repeats its position: atan2(0, 0)), the positions rounded
    through float32.  Holes, one long gap, lost rows and the width / height kinds as in make_table.  The headings of such
    a table, and the turns between them, sit exactly on whole degrees and on histogram edges again and again (steps along
    the axes and the diagonals): an atan2 that is an ulp off shows."""
    rng = np.random.default_rng(seed)
    parts = []
    for tid in range(n_tracks):
        n = int(rng.integers(40, max_len))
        t0 = int(rng.integers(0, 200))
        keep, w, h, deg, lost = _shapes_and_holes(rng, n)
        step = rng.integers(-4, 5, (n, 2)).astype(np.float64)
        step[rng.random(n) < 0.08] = 0.0                             # with the 1 in 81 drawn as (0, 0): about one in ten
        start = np.round(np.array([rng.uniform(0.1, 0.9) * width, rng.uniform(0.1, 0.9) * height]) / grid)
        xy = ((np.cumsum(step, axis=0) + start) * grid).astype(np.float32).astype(np.float64)[keep]
        m = len(xy)
        parts.append(pd.DataFrame({"TRACK_ID": np.full(m, tid, np.uint32), "POSITION_T": (t0 + np.flatnonzero(keep)).astype(np.uint32),
                                   "POSITION_X": xy[:, 0], "POSITION_Y": xy[:, 1], "WIDTH": w, "HEIGHT": h, "DEGREES_ANGLE": deg}))
    return pd.concat(parts, ignore_index=True)


def raw_centroid_table(seed, n_tracks=40, max_len=300, height=400, width=600):
    """Tracks of raw-centroid-like positions: the float32 centres of randomly rotated rectangles (the mean of four float32
    corners, as minAreaRect forms it), widened to double.  Off the 0.5 lattice, but every step is an exact difference of
    float32 values -- few significant bits, unlike a float64 random walk."""
    rng = np.random.default_rng(seed)
    parts = []
    for tid in range(n_tracks):
        n = int(rng.integers(40, max_len))
        t0 = int(rng.integers(0, 200))
        keep, w, h, deg, lost = _shapes_and_holes(rng, n)
        centre = np.cumsum(rng.normal(0, 1.2, (n, 2)), axis=0) + (rng.uniform(0.1, 0.9) * width, rng.uniform(0.1, 0.9) * height)
        centre[rng.random(n) < 0.1] = np.nan                          # lost: repeats the position before it
        centre[0] = np.nan_to_num(centre[0], nan=200.0)
        centre = pd.DataFrame(centre).ffill().to_numpy()
        th = rng.uniform(0, np.pi, n)
        hw, hh = rng.uniform(2, 5, n), rng.uniform(0.5, 2, n)
        corners = np.zeros((n, 4, 2), np.float32)
        for c, (sa, sb) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            corners[:, c, 0] = np.round(centre[:, 0] + sa * hw * np.cos(th) - sb * hh * np.sin(th))      # contour points are pixels
            corners[:, c, 1] = np.round(centre[:, 1] + sa * hw * np.sin(th) + sb * hh * np.cos(th))
        wobble = np.float32(rng.normal(0, 0.3, (n, 4, 2)))                                                # the fitted box is not on them
        xy = ((corners + wobble).sum(axis=1, dtype=np.float32) * np.float32(0.25)).astype(np.float64)[keep]
        m = len(xy)
        parts.append(pd.DataFrame({"TRACK_ID": np.full(m, tid, np.uint32), "POSITION_T": (t0 + np.flatnonzero(keep)).astype(np.uint32),
                                   "POSITION_X": xy[:, 0], "POSITION_Y": xy[:, 1], "WIDTH": w, "HEIGHT": h, "DEGREES_ANGLE": deg}))
    return pd.concat(parts, ignore_index=True)


_COLUMNS = ("TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE")


def dust_table(real, n_rows_total, seed, height=400, width=600):
    """`real` (a make_table result) with equal blocks of 2-row 'dust' tracks in front of each of its tracks: block, real
    track, block, real track, ...; the table ends with a real track.  Dust tracks have frames 0 and 1, positions anywhere
    in the frame, WIDTH in 4..8 and HEIGHT in 1..3 (an area median like any track's: they fall to the length rule of
    the clean-up, after their medians were worked out).  Ids ascend through the whole table -- a real track's becomes
    (its rank + 1) * (block + 1) - 1 -- and the block is the smallest that gives at least `n_rows_total` rows."""
    rng = np.random.default_rng(seed)
    rank = np.unique(real["TRACK_ID"].to_numpy(), return_inverse=True)[1].astype(np.int64)
    n_real = int(rank.max()) + 1
    block = max(0, -(-(int(n_rows_total) - len(real)) // (2 * n_real)))
    n_dust = block * n_real
    dust_id = np.arange(n_dust, dtype=np.int64)
    dust_id += dust_id // max(block, 1)                               # one id left free behind every block
    ids = np.concatenate([np.repeat(dust_id, 2), (rank + 1) * (block + 1) - 1])
    order = np.argsort(ids, kind="stable")
    dust = {"POSITION_T": np.tile(np.array([0, 1], np.uint32), n_dust),
            "POSITION_X": rng.uniform(0.0, width, 2 * n_dust), "POSITION_Y": rng.uniform(0.0, height, 2 * n_dust),
            "WIDTH": rng.uniform(4.0, 8.0, 2 * n_dust), "HEIGHT": rng.uniform(1.0, 3.0, 2 * n_dust),
            "DEGREES_ANGLE": rng.uniform(-90.0, 0.0, 2 * n_dust)}
    out = {"TRACK_ID": ids[order].astype(np.uint32)}
    for name in _COLUMNS[1:]:
        out[name] = np.concatenate([dust[name], real[name].to_numpy()])[order]
    return pd.DataFrame(out)


def with_wrapping_spans(real, spans=(65566, 65546)):
    """`real` behind one 2-row track per entry of `spans`, frames (0, span - 1); the real tracks' ids move up.  A span of
    65,536 frames or more does not fit the uint16 the reference keeps it in (track_eval.py:655-659): 65,566 counts as
    30 frames, 65,546 as 10."""
    k = len(spans)
    rng = np.random.default_rng(1)
    head = pd.DataFrame({"TRACK_ID": np.repeat(np.arange(k, dtype=np.uint32), 2),
                         "POSITION_T": np.array([f for s in spans for f in (0, s - 1)], np.uint32),
                         "POSITION_X": rng.uniform(100, 500, 2 * k), "POSITION_Y": rng.uniform(100, 300, 2 * k),
                         "WIDTH": rng.uniform(4, 8, 2 * k), "HEIGHT": rng.uniform(1, 3, 2 * k),
                         "DEGREES_ANGLE": rng.uniform(-90, 0, 2 * k)})
    tail = real.copy()
    tail["TRACK_ID"] = (tail["TRACK_ID"] + k).astype(np.uint32)
    return pd.concat([head, tail], ignore_index=True)


def tracker_shaped(n, n_tracks, seed):
    """(track_id, frame) of `n` rows as the link emits them: ids 0 .. n_tracks - 1, every track with a row in every frame
    from its first to its last, rows frame by frame and ids ascending within a frame."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), n_tracks - 1, replace=False)) if n_tracks > 1 else np.zeros(0, np.int64)
    lengths = np.diff(np.r_[0, cuts, n])
    first = rng.integers(0, 25, n_tracks)
    ids = np.repeat(np.arange(n_tracks), lengths)
    frames = np.concatenate([f + np.arange(m) for f, m in zip(first, lengths)])
    order = np.lexsort((ids, frames))
    return ids[order].astype(np.int64), frames[order].astype(np.int64)


def value_mix_rows(n, seed=33):
    """`n` ordered rows (200 per track) of mixed values for the device formatter's tests: uniform and float32-widened
    doubles, ties, halves, negative values, zeros, the neighbours of powers of two.  Their lines have many lengths."""
    from ysmr_amd import _lib
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, _lib.ROW_DTYPE)
    rows["track_id"] = np.arange(n) // 200
    rows["frame"] = np.arange(n) % 200
    powers = np.ldexp(1.0, np.arange(-20, 24))
    edge = np.concatenate([powers, np.nextafter(powers, 0)[1:], np.nextafter(powers, np.inf), [0.0, -0.0, 0.1, 0.5, 1e-5, 123456.789]])
    rows["x"] = np.where(rng.random(n) < 0.5, rng.uniform(-5, 1300, n), rng.uniform(0, 4000, n).astype(np.float32).astype(np.float64))
    rows["x"][:len(edge)] = edge
    rows["y"] = rng.integers(0, 4000, n) + rng.choice([0, 0.5, 0.25, 0.125, 0.1, 0.3], n)
    rows["w"], rows["h"] = rng.uniform(0, 40, n).astype(np.float32), rng.uniform(0, 40, n).astype(np.float32)
    rows["angle"] = rng.uniform(-90, 90, n).astype(np.float32)
    return rows


def select_settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False,
                            "log to file": False, "minimal length in seconds": 1.0,
                            "limit track length to x seconds": 3.0, "store processed .csv file": False})
    s.update(kw)
    return s


#: track lengths that start a track on the last row of a 2048-row scan tile (csrc/prim.h: SCAN_TILE), on the first row of the next
#: tile and on the first row of the third: rows 2047, 2079, 4096 and rows 2048, 4096
TILE_EDGE_LENGTHS = ((2047, 32, 2017, 40), (2048, 2048, 40))


def walk_table(lengths, seed=9):
    """Random-walk tracks of the given lengths, one after the other, every frame present."""
    rng = np.random.default_rng(seed)
    parts = []
    for tid, n in enumerate(lengths):
        xy = np.cumsum(rng.normal(0, 1.5, (n, 2)), axis=0) + 300
        parts.append(pd.DataFrame({"TRACK_ID": np.full(n, tid, np.uint32), "POSITION_T": np.arange(n, dtype=np.uint32),
                                   "POSITION_X": xy[:, 0], "POSITION_Y": xy[:, 1], "WIDTH": rng.uniform(4, 8, n),
                                   "HEIGHT": rng.uniform(1, 3, n), "DEGREES_ANGLE": rng.uniform(0, 90, n)}))
    return pd.concat(parts, ignore_index=True)
