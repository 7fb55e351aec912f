"""Synthetic detection clips for the 3-D batch link -- test helper, not collected.

``clip3`` makes blobs that drift over a 1228 x 922 field with a luminosity level each; ``model_table`` runs
tests/luminosity_model.py::Linker over them.  No images are involved: the clips are lists of detections, which is what
``ysmr_tracker_run3`` takes.
"""
import functools

import numpy as np

import luminosity_model as M

WIDTH, HEIGHT = 1228.0, 922.0
MAX_DISAPPEARED = 5.0
#: second word of the generator's seed.  Chosen on the MODEL alone (the lowest for which every clip the tests use meets their
#: two preconditions -- the third coordinate decides an identity, no decision hangs on a gap below 1e-9): on most streams
#: the 120 blobs at scale 1 never come near enough to each other for a luminosity difference of 2 to matter
STREAM = 6


@functools.lru_cache(maxsize=None)
def clip3(n_frames, n_blobs, seed, scale):
    """-> tuple of per-frame (points f64 [m][3] = x, y, luminosity; infos f32 [m][3] = w, h, angle).

    Uniform start positions, velocity N(0, 0.8) plus N(0, 0.3) jitter per frame; a luminosity level per blob,
    U(0.4, 2.4) * scale, plus N(0, 0.02 * scale) per frame; 10 % of the blobs appear late and 10 % leave early; 2 %
    dropout except in every seventh frame (so that frames with more detections than tracks -- births -- happen); x and y
    rounded to float32 (a detector's output); the detections of a frame shuffled."""
    rng = np.random.default_rng((seed, STREAM))
    pos = np.stack([rng.uniform(0, WIDTH, n_blobs), rng.uniform(0, HEIGHT, n_blobs)], 1)
    vel = rng.normal(0.0, 0.8, (n_blobs, 2))
    level = rng.uniform(0.4, 2.4, n_blobs) * scale
    first = np.zeros(n_blobs, np.int64)
    last = np.full(n_blobs, n_frames, np.int64)
    late = rng.choice(n_blobs, n_blobs // 10, replace=False)
    first[late] = rng.integers(2, max(n_frames // 2, 3), len(late))
    rest = np.setdiff1d(np.arange(n_blobs), late)
    early = rng.choice(rest, n_blobs // 10, replace=False)
    last[early] = rng.integers(max(n_frames // 2, 3), n_frames - 1, len(early))
    box = np.stack([rng.uniform(2, 9, n_blobs), rng.uniform(2, 9, n_blobs), rng.uniform(0, 90, n_blobs)], 1).astype(np.float32)
    frames = []
    for f in range(n_frames):
        pos = pos + vel + rng.normal(0.0, 0.3, (n_blobs, 2))
        lum = level + rng.normal(0.0, 0.02 * scale, n_blobs)
        seen = (first <= f) & (f < last)
        if f % 7:
            seen &= rng.uniform(size=n_blobs) >= 0.02
        idx = np.flatnonzero(seen)
        rng.shuffle(idx)
        pts = np.empty((len(idx), 3))
        pts[:, :2] = pos[idx].astype(np.float32)
        pts[:, 2] = lum[idx]
        frames.append((pts, box[idx].copy()))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def model_table(n_frames, n_blobs, seed, scale, dims=3):
    """The model's table of a clip: (rows per frame [[(frame, id, x, y, w, h, deg, disappeared)]], ids / points / counters
    after the last frame, next id, the linker's min_gap, the largest number of live tracks)."""
    lk = M.Linker(MAX_DISAPPEARED)
    per_frame, most = [], 0
    for f, (pts, box) in enumerate(clip3(n_frames, n_blobs, seed, scale)):
        lk.update(pts[:, :dims], [tuple(float(v) for v in b) for b in box])
        per_frame.append(lk.rows(f))
        most = max(most, len(lk.objects))
    ids = list(lk.objects.keys())
    pts = np.array([lk.objects[i] for i in ids]).reshape(-1, dims)
    gone = [lk.disappeared[i] for i in ids]
    return per_frame, (ids, pts, gone), lk.next_id, lk.min_gap, most


def identities_differ(table_a, table_b):
    """Some track's rows (frames and positions) differ between two per-frame tables."""
    def by_id(per_frame):
        out = {}
        for rows in per_frame:
            for r in rows:
                out.setdefault(r[1], []).append((r[0], r[2], r[3]))
        return out
    return by_id(table_a) != by_id(table_b)


def arrays(frames, max_det, stale=True):
    """A clip as ``run`` takes it: det f32 [F][max_det][5], third f64 [F][max_det], counts i32 [F].  stale: slots at or
    beyond a frame's count hold plausible values -- the position and the luminosity of the frame's first detection -- and
    must not be read."""
    n = len(frames)
    det = np.zeros((n, max_det, 5), np.float32)
    third = np.full((n, max_det), 7.0)
    counts = np.zeros(n, np.int32)
    for f, (pts, box) in enumerate(frames):
        m = len(pts)
        counts[f] = m
        det[f, :m, :2], det[f, :m, 2:] = pts[:, :2], box
        third[f, :m] = pts[:, 2]
        if stale and m:
            det[f, m:, :2] = pts[0, :2]
            det[f, m:, 2:] = box[0]
            third[f, m:] = pts[0, 2]
    return det, third, counts
