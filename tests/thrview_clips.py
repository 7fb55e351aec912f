"""The clip of the threshold view's end-to-end tests and what the CPU oracle says its pictures are.  13 frames of 96 x 80:
twelve rods of ysmr_amd/synth.py, every third of them faint (peak 54 on a background of 40), so that in every frame some
pixels are kept markers, some are kept without being markers (the rim of a bright rod, or a faint rod that touches one) and
some pass the low threshold and are dropped by the hysteresis (a faint rod alone).  Computed once, never modified."""
import functools

import numpy as np

import thrview_model as T

H, W, FRAMES, BATCH, FPS = 80, 96, 13, 4, 30.0         # three full batches and a last one of one frame


@functools.lru_cache(maxsize=None)
def clip(kind):
    """'gray': u8 [13, 80, 96]; 'bgr': the same scene with three different channels, u8 [13, 80, 96, 3]."""
    from ysmr_amd.synth import SyntheticVideo
    video = SyntheticVideo(H, W, 12, seed=3, dropout=0.0, speckle=0.0)
    video.peak[::3] = 54.0
    frames = video.frames(FRAMES)
    if kind == "bgr":
        wide = frames.astype(np.int32)
        frames = np.stack([np.clip(wide - 3, 0, 255), wide, np.clip(wide * 9 // 10 + 6, 0, 255)], axis=3).astype(np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def oracle_maps(kind, adt=2.0):
    """(cls, mask) u8 [13, 80, 96] of the clip as oracle/ysmr_oracle.py computes them on the CPU, frame by frame: the class map
    and the mask behind the hysteresis, for 'threshold offset for detection' = 5 on white-on-dark frames and this 'adaptive
    double threshold' (below 0: the mean-gray branch, whose level runs through the clip)."""
    from oracle import ysmr_oracle as yo
    yo.build()
    frames = clip(kind)
    levels = yo.MeanGrayLevels(FPS, True, 5) if adt < 0 else None
    cls, mask = [], []
    for frame in frames:
        fd = yo.detect_frame_mean_gray(frame, levels) if levels is not None else yo.detect_frame(frame, *yo.threshold_params(True, 5, adt))
        cls.append(fd.cls)
        mask.append(fd.mask)
    cls, mask = np.stack(cls), np.stack(mask)
    cls.setflags(write=False)
    mask.setflags(write=False)
    return cls, mask


def expected(kind, mode, adt=2.0):
    """The pictures u8 [13, 80, 96, 3] the view has to store for the clip."""
    cls, mask = oracle_maps(kind, adt)
    return T.paint(clip(kind), cls, mask, T.MODES[mode])


def classes_per_frame(kind, adt=2.0):
    """[13, 3] pixel counts per frame: kept markers, kept without a marker, dropped by the hysteresis -- from the oracle's maps."""
    cls, mask = oracle_maps(kind, adt)
    kept = mask != 0
    return np.stack([(kept & (cls & 2 != 0)).sum(axis=(1, 2)), (kept & (cls & 2 == 0)).sum(axis=(1, 2)),
                     (~kept & (cls & 1 != 0)).sum(axis=(1, 2))], axis=1)
