"""tests/cell_list_model.py -- the float32 statement of k_bgrid's candidate lists -- held to brute force, and the clips of
tests/split_clips.py to what their GPU test is about.  No GPU needed.

The lists' promise (csrc/batch_link.h, above bl_rect_list): for every point p of the grown rectangle the list holds the
float64 argmin over all detections, and every detection bl_search's float tie band can reach from it.  The band in exact
squared distances: bl_search keeps what lies within best + 0.2 + 5e-6 best of the best FLOAT distance, and a float distance
is off by at most 0.1 + 3e-6 s, so a detection d can enter only with
    s_d (1 - 3e-6) - 0.1 <= (s_min (1 + 3e-6) + 0.1) (1 + 5e-6) + 0.2,   i.e.   s_d <= (1 + 1.2e-5) s_min + 0.41
(for s below 1e6 px^2) -- that is what must be listed; the pruning's own margin, (1 + 3e-5) s + 0.6, lies above it.
"""
import numpy as np
import pytest

import cell_list_model as M
from split_clips import split_clip


def _points(rect, rng, n):
    ax, bx, ay, by = (float(v) for v in rect)
    p = np.column_stack([rng.uniform(ax, bx, n), rng.uniform(ay, by, n)])
    corners = np.array([[ax, ay], [bx, ay], [ax, by], [bx, by], [0.5 * (ax + bx), 0.5 * (ay + by)]])
    return np.vstack([corners, p])


def _check(g, xy, cx, cy, rect, rng, n=120):
    kept, gathered = M.rect_list(g, xy, cx, cy, rect)
    if M.flagged(kept):
        return False
    p = _points(rect, rng, n)
    d = xy.astype(np.float64)
    s = (p[:, None, 0] - d[None, :, 0]) ** 2 + (p[:, None, 1] - d[None, :, 1]) ** 2
    need = s <= (1 + 1.2e-5) * s.min(axis=1, keepdims=True) + 0.41
    listed = np.zeros(len(d), bool)
    listed[kept] = True
    missing = need & ~listed[None, :]
    assert not missing.any(), f"cell ({cx}, {cy}) rect {rect}: detections {np.flatnonzero(missing.any(0))} not in {kept}"
    assert kept == sorted(kept) and len(kept) >= 1
    return True


def _frames():
    rng = np.random.default_rng(11)
    out = [split_clip(16)[0][k][0] for k in (0, 1)] + [split_clip(32)[0][k][0] for k in (1, 5)]
    out.append(np.column_stack([rng.uniform(10, 1218, 520), rng.uniform(10, 912, 520)]))       # a frame like the bench's
    out.append(rng.uniform(600, 640, (60, 2)))                                                  # one dense cluster
    return [np.asarray(a, np.float32) for a in out]


@pytest.mark.parametrize("k", range(6))
def test_lists_hold_the_nearest_and_its_tie_band(k):
    rng = np.random.default_rng(100 + k)
    xy_in = _frames()[k]
    g, order = M.bin_frame(xy_in)
    xy = xy_in[order]
    G = g.G
    cells = set(rng.choice(G * G, 60, replace=False).tolist())
    cells |= set(np.flatnonzero(np.diff(g.start) > 0)[:40].tolist())          # and cells that hold detections
    checked = quads = 0
    for c in sorted(cells):
        cx, cy = c % G, c // G
        if _check(g, xy, cx, cy, M.cell_rect(g, cx, cy), rng):
            checked += 1
        else:                      # a crowded cell: its quadrants
            for q in range(4):
                quads += _check(g, xy, cx, cy, M.quad_rect(g, cx, cy, q), rng)
    assert checked >= 40
    # every crowded cell of the frame, not only the sampled ones
    if k < 4:
        detail = {}
        M.frame_lists(g, xy, detail=detail)
        for c in detail:
            for q in range(4):
                quads += _check(g, xy, c % G, c // G, M.quad_rect(g, c % G, c // G, q), rng)
        assert quads >= 4


def test_quadrants_tile_the_cell_and_share_its_sides():
    g, _ = M.bin_frame(split_clip(32)[0][1][0])
    for cx, cy in ((0, 0), (5, 6), (31, 31), (17, 2)):
        ax, bx, ay, by = M.cell_rect(g, cx, cy)
        q = [M.quad_rect(g, cx, cy, k) for k in range(4)]
        assert q[0][0] == q[2][0] == ax and q[1][1] == q[3][1] == bx and q[0][2] == q[1][2] == ay and q[2][3] == q[3][3] == by
        e = M.grow(g)
        # (the halves overlap by 2 e across the midline, to the rounding of a coordinate below 2048: 1.2e-4 px)
        assert q[0][1] - q[1][0] == pytest.approx(2 * float(e), abs=5e-4) and q[0][3] - q[2][2] == pytest.approx(2 * float(e), abs=5e-4)


def test_lane_side_quadrant_lies_in_its_grown_rectangle():
    """What bl_search decides in float for a float64 prediction -- cell and quadrant -- is a rectangle that holds it."""
    rng = np.random.default_rng(5)
    g, _ = M.bin_frame(split_clip(32)[0][1][0])
    e = float(M.grow(g))
    cell, x0, y0 = float(g.cell), float(g.x0), float(g.y0)
    pts = rng.uniform(0, 1500, (400, 2))
    # and points a hair from cell borders and midlines
    k = rng.integers(0, 2 * g.G, (400, 2))
    near = np.column_stack([x0 + 0.5 * cell * k[:, 0], y0 + 0.5 * cell * k[:, 1]]) + rng.uniform(-1, 1, (400, 2)) * 1e-3 * rng.choice([0, 1e-3, 1], (400, 1))
    for px, py in np.vstack([pts, near]):
        cx, cy, q = M.lane_cell(g, px, py)
        if not (0 <= cx < g.G and 0 <= cy < g.G):
            continue
        ax, bx, ay, by = (float(v) for v in M.quad_rect(g, cx, cy, q))
        assert ax <= px <= bx and ay <= py <= by, (px, py, cx, cy, q)


@pytest.mark.parametrize("G", [16, 32])
def test_split_clip_holds_what_its_gpu_test_is_about(G):
    frames, rings = split_clip(G)
    counts = [len(xy) for xy, _ in frames]
    assert all(M.grid_n(m) == G for m in counts) and (max(counts) <= 128 if G == 16 else 160 <= max(counts) <= 300)
    f = 5 if G == 32 else 1
    xy = np.asarray(frames[f][0], np.float32)
    g, order = M.bin_frame(xy)
    detail = {}
    lists, over = M.frame_lists(g, xy[order], detail=detail)
    split, flag = lists[:, 0] == M.SPLIT, lists[:, 0] == M.FLAG
    assert split.sum() >= 2 and flag.sum() >= 1
    if G == 32:
        assert len(detail) > M.BL_OVF and split.sum() <= M.BL_OVF          # more crowded cells than entries
    # the ring of equal radii: its cell stays flagged although it has an entry (every quadrant still holds all twelve)
    eq = next(c for c, _, equal, _ in rings if equal)
    cx, cy, _ = M.lane_cell(g, *eq)
    c = cy * G + cx
    assert flag[c] and sorted(detail).index(c) < M.BL_OVF and all(M.flagged(q) for q in detail[c][2])
    # the probes of the frame before are this frame's predictions (GSFF off): in split cells, in every quadrant, and some
    # within e of a midline on either side of it
    assert (f - 1) % 2 == 0
    probes = frames[f - 1][0][-8 * sum(always for _, _, _, always in rings):]
    where = [M.lane_cell(g, px, py) for px, py in probes]
    in_split = [(cx, cy, q) for cx, cy, q in where if split[cy * G + cx]]
    assert len(in_split) >= 8 and {q for _, _, q in in_split} == {0, 1, 2, 3}
    e = float(M.grow(g))
    ux = (probes[:, 0] - float(g.x0)) / float(g.cell) % 1.0 - 0.5
    assert (np.abs(ux) * float(g.cell) <= e).sum() >= 4 and (ux == 0).sum() >= 1


def test_block_layout_is_the_librarys(tmp_path):
    """grid_n, list_off, ovf_off and grid_dwords here against csrc/tracker_plan.h's bl_grid_n, bl_list_off, bl_ovf_off and
    bl_grid_dwords, for every detection count k_bgrid serves (tests/tracker_plan_check.cc prints them; no GPU needed)."""
    from test_tracker_plan_sanitized import run_plan_check
    rows = [tuple(int(v) for v in line.split()[1:]) for line in run_plan_check(tmp_path) if line.startswith("grid ")]
    assert [r[0] for r in rows] == list(range(2561))
    for m, n, list_off, ovf_off, dwords in rows:
        assert (M.grid_n(m), M.list_off(m), M.ovf_off(m), M.grid_dwords(m)) == (n, list_off, ovf_off, dwords), m
