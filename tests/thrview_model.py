"""The threshold view's pixel rule in NumPy ('hip save threshold video', csrc/thrview_rule.h): a few ``np.where`` over the
class map (bit 0 thresh, bit 1 markers), the final mask and, in mode 2, the frame.  ``paint`` gives the pictures,
``stored`` the DIB frames they are kept as."""
import numpy as np

import annotate_model as A

MASK, MARKERS, CLASSES = 0, 1, 2
MODES = {"mask": MASK, "markers": MARKERS, "classes": CLASSES}
KEPT_MARKER, KEPT, DROPPED = (0, 0, 255), (0, 255, 255), (255, 0, 0)          # B, G, R

#: the shapes (n, H, W) every test of the kernel and of its host twin goes through: a row shorter than one lane's step of 16
#: pixels, one pixel, exactly one step, a tail of 15, a tail that starts at an odd address, more than one wave's 1024 pixels
SHAPES = ((1, 1, 1), (3, 3, 5), (2, 5, 16), (2, 4, 63), (1, 7, 67), (2, 3, 1040))


def paint(frames, cls, mask, mode):
    """u8 [n, H, W, 3] (B, G, R) from cls, mask u8 [n, H, W] and -- mode 2 only -- frames u8 [n, H, W] or [n, H, W, 3]."""
    cls, kept = np.asarray(cls), None if mask is None else np.asarray(mask) != 0
    if mode == MASK:
        return np.repeat(np.where(kept, 255, 0).astype(np.uint8)[..., None], 3, axis=3)
    if mode == MARKERS:
        return np.repeat(np.where(cls & 2, 255, 0).astype(np.uint8)[..., None], 3, axis=3)
    assert mode == CLASSES
    out = A.to_bgr(frames)
    out[~kept & (cls & 1 != 0)] = DROPPED
    out[kept & (cls & 2 == 0)] = KEPT
    out[kept & (cls & 2 != 0)] = KEPT_MARKER
    return out


def stored(frames, cls, mask, mode, stride=None, bottom_up=0, frame_bytes=None, fill=0):
    """The stored frames u8 [n, frame_bytes]: rows ``stride`` apart, padding zero, bytes behind a frame's last row ``fill``."""
    return A.pack_dib(paint(frames, cls, mask, mode), bottom_up, stride, frame_bytes, fill)


def random_maps(rng, shape):
    """cls in 0 .. 7 and mask in {0, 255}, independent: every combination of (cls & 3, mask != 0) is likely from 64 pixels on."""
    return rng.integers(0, 8, shape, dtype=np.uint8), (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)


def combinations(cls, mask):
    """The set of (cls & 3, mask != 0) that occur."""
    return set(zip((np.asarray(cls) & 3).reshape(-1).tolist(), (np.asarray(mask) != 0).reshape(-1).tolist()))
