"""Clips and expected tables for the luminosity tests -- test helper, not collected.

``crossing_clip``: a small synthetic recording of PAIRS of blobs of unlike peak brightness that pass within two pixels
of each other -- the situation 'include luminosity in tracking calculation' exists for.  (The third coordinate is a mean gray
value / 100, so it weighs little against pixels: the defaults below -- fast blobs, peaks of 70-90 against 205-245 -- were
chosen so that it decides at least one identity on both threshold branches; the tests assert that on the expected data.)

``expected_rows``: what the reference's frame loop makes of a clip with that setting on and the GSFF off -- the oracle's
detection, the model's luminosity (tests/luminosity_model.py) and the model's linker; with ``dims=2`` the same without
the third coordinate.
"""
import numpy as np

import luminosity_model as M


def crossing_clip(height=240, width=320, n_frames=72, n_pairs=16, seed=5, background=40.0, noise=2.0):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(40, width - 40, n_pairs), rng.uniform(40, height - 40, n_pairs)], 1)
    ang = rng.uniform(0, np.pi, n_pairs)
    t_cross = rng.integers(12, n_frames - 12, n_pairs)
    speed = rng.uniform(1.5, 3.0, n_pairs)
    off = rng.uniform(1.0, 2.0, n_pairs)
    peak = np.stack([rng.uniform(70, 90, n_pairs), rng.uniform(205, 245, n_pairs)], 1)
    radius = rng.uniform(1.2, 1.9, (n_pairs, 2))
    gy, gx = np.mgrid[-4:5, -4:5]
    frames = np.empty((n_frames, height, width), np.uint8)
    for f in range(n_frames):
        img = rng.normal(background, noise, (height, width))
        signal = np.zeros((height, width))
        d = np.stack([np.cos(ang), np.sin(ang)], 1)
        nrm = np.stack([-d[:, 1], d[:, 0]], 1)
        s = ((f - t_cross) * speed)[:, None]
        for k, pos in enumerate((c + d * s + nrm * off[:, None] / 2, c - d * s - nrm * off[:, None] / 2)):
            for p in range(n_pairs):
                ci = np.rint(pos[p]).astype(int)
                dist = np.hypot(gx - (pos[p, 0] - ci[0]), gy - (pos[p, 1] - ci[1]))
                val = np.clip(0.5 - (dist - radius[p, k]), 0.0, 1.0) * (peak[p, k] - background)
                yy, xx = gy + ci[1], gx + ci[0]
                ok = (val > 0) & (yy >= 0) & (yy < height) & (xx >= 0) & (xx < width)
                np.maximum.at(signal, (yy[ok], xx[ok]), val[ok])
        frames[f] = np.clip(np.rint(img + signal), 0, 255).astype(np.uint8)
    return frames


def expected_rows(oracle, frames, fps, dims=3, white_on_dark=True, offset=5, adt=2.0):
    """-> (rows [(frame, id, x, y, w, h, deg, disappeared)], the model linker after the last frame)."""
    mean_gray = oracle.MeanGrayLevels(fps, white_on_dark, offset) if adt < 0 else None
    if mean_gray is None:
        inv, t_low, t_high, use_high = oracle.threshold_params(white_on_dark, offset, adt)
    lk = M.Linker(fps)           # track_bacteria: max_disappeared = fps (track_eval.py:136-144)
    rows = []
    for k, frame in enumerate(frames):
        fd = oracle.detect_frame(frame, inv, t_low, t_high, use_high) if mean_gray is None else \
            oracle.detect_frame_mean_gray(frame, mean_gray)
        gray = frame if frame.ndim == 2 else M.bgr2gray(frame)
        lum = M.luminosity_frame(gray, fd.det)[3]
        pts = np.column_stack([fd.det[:, 0].astype(np.float64), fd.det[:, 1].astype(np.float64), lum])[:, :dims]
        lk.update(pts, [tuple(float(v) for v in d[2:5]) for d in fd.det])
        rows.extend(lk.rows(k))
    return rows, lk


def tracks_differ(rows_a, rows_b):
    """At least one track's rows (its frames and positions) differ between two tables."""
    def by_id(rows):
        out = {}
        for r in rows:
            out.setdefault(r[1], []).append((r[0], r[2], r[3]))
        return out
    return by_id(rows_a) != by_id(rows_b)
