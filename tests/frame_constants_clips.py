"""Detection sequences for tests/test_gpu_batch_frame_constants.py: what the batch link can get wrong once a frame's count
and grid header are read a frame AHEAD (csrc/batch_link.h, k_batch, above the frame loop).

Pure numpy, as tests/one_barrier_clips.py: stationary lattice points and no filter bank, so k_batch in launches of any
length, the per-frame link and the host tracker must give EQUAL rows.  Every frame shows a subset of ONE fixed set of 760
lattice points (table capacity 768): a window of the frame's count that starts a little further round the set with every
frame, so that frames register beside live tracks, tracks lose their point and propose a neighbour's, and die."""
import numpy as np

from one_barrier_clips import _frame, lattice

POINTS = 760
# The counts change the shape of the frame's grid block from one frame to the next: cells per side G = 16 up to 128
# detections, 32 up to 600, 48 above (bl_grid_n); candidate lists for G <= 32 only (bl_has_lists); no block at all for an
# empty frame.  601 -> 601 keeps the shape, 601 -> 0 -> 1 goes through an empty frame into the smallest, 128 -> 129 and
# 600 -> 601 step over a threshold, 601 -> 130 and 1 -> 601 (the wrap) jump two shapes, 0 -> 0 stays empty.
COUNTS = (601, 601, 0, 1, 128, 129, 600, 601, 130, 0, 0, 601, 1)
REPEATS = 7      # 13 and 7 are coprime: over 7 repeats (and one frame more, for the last wrap) every change falls once on
                 # every frame of a 7-frame launch -- on its last frame and the first frame of the next among them
STRIDE = 37      # points the window moves on per frame


def grid_shape(m):
    """(cells per side, candidate lists) of a frame with m detections; (0, False) for an empty frame."""
    if m == 0:
        return 0, False
    g = 16 if m <= 128 else 32 if m <= 600 else 48
    return g, g <= 32


def shape_changes_clip():
    pts = lattice(POINTS)
    counts = COUNTS * REPEATS + COUNTS[:1]
    frames = []
    for f, m in enumerate(counts):
        first = (STRIDE * f) % POINTS
        frames.append(_frame([pts[(first + i) % POINTS] for i in range(m)], 900 + f))
    return frames, counts


def full_frames_clip(n_frames, m):
    """`n_frames` frames of the same m lattice points: for hand-made counts above and below what the frames hold."""
    pts = lattice(m)
    return [_frame(pts, 950 + f) for f in range(n_frames)]
