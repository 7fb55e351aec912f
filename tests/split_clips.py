"""Detection sequences for the split candidate lists (csrc/batch_link.h: k_bgrid gives a cell whose list overflows the
lists of its four quadrants).  Pure numpy; tests/test_cell_list_model.py checks with the model that a clip holds what its
GPU test (tests/test_gpu_cell_lists_split.py) is about.

A clip fixes its grid with two anchor detections at (0, 0) and (E, E): the cells are E / (G - 2) wide and cell (i, j) has
its centre at ((i - 0.5) cell, (j - 0.5) cell).  Around such centres lie RINGS of 9 .. 14 detections at slightly different
radii, the patch inside empty: every member is the nearest somewhere in the cell, the list overflows, the quadrants' lists
do not.  One ring of 12 has equal radii: all twelve are nearest at the centre, which every grown quadrant contains, so its
cell stays flagged.  Frames alternate: a frame WITH probes (detections inside the patches: on the midlines of the cell,
within e = 4e-3 px + 2e-4 cells of them on either side, changing sides from one probe frame to the next) hands their tracks
a position, the frame after it, without them, has those tracks' predictions in the crowded cells.  One frame without
probes shows every ring: more crowded cells than overflow entries.
"""
import numpy as np


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64).reshape(-1, 2)


def _info(rng, n):
    return np.asarray(np.column_stack([rng.uniform(1, 9, n), rng.uniform(1, 9, n), rng.uniform(0, 90, n)]), np.float32).astype(np.float64)


def _ring(rng, c, r, k, equal):
    a = 2 * np.pi * (np.arange(k) + (0.0 if equal else rng.uniform(0, 1))) / k
    rad = np.full(k, r) if equal else r + rng.permutation(k) * 0.35 + rng.uniform(0, 0.1, k)
    return np.column_stack([c[0] + rad * np.cos(a), c[1] + rad * np.sin(a)])


def _probes(c, e, side):
    """Eight detections inside the patch around the cell's centre c: on the midlines, within e of them on the side `side` (+1 / -1)."""
    h = 0.5 * e * side
    return np.array([[c[0], c[1] - 9.0], [c[0] + h, c[1] + 9.0], [c[0] - h, c[1] + 17.0], [c[0] - 2 * e * side, c[1] - 17.0],
                     [c[0] - 13.0, c[1]], [c[0] + 13.0, c[1] + h], [c[0] + 21.0, c[1] - h], [c[0] - 21.0, c[1] + 2 * e * side]])


def split_clip(G, seed=3):
    """[(xy (m, 2), info (m, 3)) per frame] for a grid of G cells per side (16: ~100-130 detections, 32: ~170-300), and the
    rings [(centre of the ring's cell, members, equal radii, shown in every frame)]."""
    rng = np.random.default_rng(seed)
    cell = 100.0 if G == 16 else 50.0
    E = cell * (G - 2)
    e = 4e-3 + 2e-4 * cell
    r0 = 0.36 * cell
    if G == 16:
        spots = [((3, 4), 9, False, True), ((9, 3), 12, True, True), ((6, 8), 14, False, True), ((11, 11), 10, False, True)]
        n_bg, n_frames, all_rings = 48, 8, None
    else:
        spots = [((5, 6), 9, False, True), ((14, 4), 12, True, True), ((9, 12), 14, False, True), ((22, 9), 11, False, True),
                 ((4, 20), 10, False, False), ((12, 22), 10, False, False), ((19, 17), 9, False, False), ((26, 24), 11, False, False),
                 ((27, 4), 10, False, False), ((18, 27), 10, False, False), ((8, 27), 9, False, False)]
        n_bg, n_frames, all_rings = 120, 10, 5
    rings = []
    for (i, j), k, equal, always in spots:
        mid = np.array([(i - 0.5) * cell, (j - 0.5) * cell])                     # the cell's centre: where its midlines cross
        rings.append((mid, _ring(rng, mid + (0.0 if equal else rng.uniform(-0.8, 0.8, 2)), r0, k, equal), equal, always))
    centres = np.array([c for c, _, _, _ in rings])
    bg = np.zeros((0, 2))
    while len(bg) < n_bg:        # background: nothing within 1.6 cells of a ring's centre
        p = rng.uniform(0.3 * cell, E - 0.3 * cell, 2)
        if np.min(np.linalg.norm(centres - p, axis=1)) > 1.6 * cell and (len(bg) == 0 or np.min(np.linalg.norm(bg - p, axis=1)) > 0.3 * cell):
            bg = np.vstack([bg, p])
    vel = rng.normal(0, 0.6, bg.shape)
    anchors = np.array([[0.0, 0.0], [E, E]])
    frames = []
    for f in range(n_frames):
        bg = bg + vel
        show_all = f == 0 or f == all_rings
        parts = [anchors, bg] + [pts for _, pts, _, always in rings if always or show_all]
        if f % 2 == 0 and f != all_rings:
            side = 1.0 if f % 4 == 0 else -1.0
            parts += [_probes(c, e, side) + (np.array([3.0, 2.0]) if equal else 0.0) for c, _, equal, always in rings if always]
        xy = _f32(np.vstack(parts))
        frames.append((xy, _info(rng, len(xy))))
    return frames, rings
