"""The batch link with a frame's constants read a frame ahead (csrc/batch_link.h, k_batch, above the frame loop): the
count of frame f + 1 and the header of its grid block are read behind barrier A of frame f and consumed at the head of the
next search; the count of frame f + 2 is read there once, for the LDS-DMA and the key clearing, and moves up a frame with
each pass.  What that can get wrong: a count or a header that belongs to the frame before or behind (every change of the
block's shape from one frame to the next, also across two launches), the prologue of a launch too short to have anything
to fetch ahead, and the clamp of a count that is no count.

Every clip (tests/frame_constants_clips.py: stationary lattice points, no filter bank, so every link must give EQUAL rows)
runs through k_batch in launches of 64 / 7 / 1 frames, through the per-frame link and through the host ``CentroidTracker``
(test_gpu_batch_claims._all_ways).  Before that the CPU oracle says that the clip does what the test is named for.

The cap on what is compared: none.  Every row of every frame of a clip is compared.
"""
import numpy as np
import pytest

import frame_constants_clips as fc
import one_barrier_clips as clips
from test_gpu_batch_claims import MAX_GONE, _all_ways, _assert_rows_equal, _run

pytestmark = pytest.mark.gpu

ERR_DET_CLAMPED = 4          # csrc/track.hip


@pytest.fixture(scope="module")
def shape_clip(oracle):
    """The clip of (a), checked on the CPU oracle: (frames, counts, live tracks per frame)."""
    frames, counts = fc.shape_changes_clip()
    assert [len(d) for d, _ in frames] == list(counts)
    births, deaths, live = clips.events(oracle, frames)
    # every change of the sequence, the wrap included, on the last frame of a 7-frame launch and the first of the next
    across = {(counts[f], counts[f + 1]) for f in range(len(counts) - 1) if f % 7 == 6}
    assert across == {(a, b) for a, b in zip(fc.COUNTS, fc.COUNTS[1:] + fc.COUNTS[:1])}
    shapes = {fc.grid_shape(m) for m in counts}
    assert shapes == {(0, False), (16, True), (32, True), (48, False)}
    # it registers beside live tracks, proposes (live tracks meet detections in every shape) and deregisters
    assert live.max() <= 768, "more tracks than the table holds"
    assert sum(1 for f, b in enumerate(births) if b and f and live[f - 1] > 0) >= 10, "registrations beside live tracks"
    assert sum(1 for d in deaths if d) >= 30
    for shape in shapes - {(0, False)}:
        assert any(fc.grid_shape(counts[f]) == shape and live[f - 1] > 0 for f in range(1, len(counts))), shape
    # tracks that lose their point propose a neighbour's: some frame ages tracks while it holds detections
    assert any(counts[f] and live[f - 1] > counts[f] for f in range(1, len(counts)))
    return frames, counts, live


@pytest.mark.parametrize("max_det", [640, 768])
def test_counts_that_change_the_blocks_shape_from_frame_to_frame(shape_clip, max_det):
    """(a): 601, 601, 0, 1, 128, 129, 600, 601, 130, 0, 0, 601, 1, seven times over: G 16 / 32 / 48, lists present and
    absent, empty frames; every change also across two launches of 7 frames."""
    frames, counts, live = shape_clip
    rows = _all_ways(frames, capacity=768, max_det=max_det)
    assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)


def _run_cuts(per_frame, cuts, max_det, capacity=768):
    """The clip through k_batch in launches of the given lengths, one after the other (the last repeats)."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker, rows_to_numpy
    trk = DeviceTracker(capacity=capacity, max_det=max_det, max_disappeared=MAX_GONE, fps=30.0, use_gsff=False)
    assert trk.batched
    cap = sum(len(d) for d, _ in per_frame) * 2 + 64
    rows = torch.empty(cap * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    b0, k = 0, 0
    while b0 < len(per_frame):
        chunk = per_frame[b0:b0 + cuts[min(k, len(cuts) - 1)]]
        det = np.zeros((len(chunk), max_det, 5), np.float32)
        for i, (d, info) in enumerate(chunk):
            det[i, :len(d)] = np.column_stack([d, info])
        cnt = torch.tensor([len(d) for d, _ in chunk], dtype=torch.int32, device="cuda")
        trk.run(torch.from_numpy(det).cuda(), cnt, b0, rows, count)
        b0 += len(chunk)
        k += 1
    torch.cuda.synchronize()
    assert trk.info()[2] == 0
    return rows_to_numpy(rows, int(count.item())).copy()


def test_launches_of_one_two_and_three_frames_on_a_fresh_and_on_a_populated_table(shape_clip):
    """(b): the prologue reads the first two frames' counts and the first header, and a launch of one frame has nothing
    to fetch ahead.  The first 26 frames of (a)'s clip (every shape, two empty stretches): a fresh table takes a first
    launch of 1, 2 and 3 frames; a populated one -- after a launch of 5 -- launches of 1, 2, 3 in turn and of each alone."""
    frames = shape_clip[0][:26]
    want = _run(_tracker(640), frames, 64, 640)
    for cuts in ((1, 64), (2, 64), (3, 64), (5, 1, 2, 3, 1, 2, 3, 3, 2, 1), (5, 1), (5, 2), (5, 3)):
        _assert_rows_equal(_run_cuts(frames, cuts, 640), want, f"launches of {cuts} frames against one launch")
    for n in (1, 2, 3):           # a clip that ENDS behind its first launch
        _assert_rows_equal(_run_cuts(frames[:n], (n,), 640), want[want["frame"] < n], f"a clip of {n} frames")


def _tracker(max_det, capacity=768):
    from ysmr_amd.tracker import DeviceTracker
    trk = DeviceTracker(capacity=capacity, max_det=max_det, max_disappeared=MAX_GONE, fps=30.0, use_gsff=False)
    assert trk.batched
    return trk


@pytest.mark.parametrize("where", ["mid-launch", "last frame of a launch"])
@pytest.mark.parametrize("word, clamped, flagged", [(64 + 1, 64, True), (-3, 0, False)])
def test_hand_made_count_is_clamped_as_before(word, clamped, flagged, where):
    """(c): a det_count word above max_det, and a negative one, through DeviceTracker.run: the rows are those of the
    clamped counts (max_det: every slot of the frame holds a detection; 0: an empty frame), ERR_DET_CLAMPED is set for the
    first and not for the second."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    max_det, n_frames, launch = 64, 14, 7
    frames = fc.full_frames_clip(n_frames, max_det)
    bad = 10 if where == "mid-launch" else 6
    shown = [(d[:clamped], info[:clamped]) if f == bad else (d, info) for f, (d, info) in enumerate(frames)]
    want = _run(_tracker(max_det, 128), shown, launch, max_det)
    assert np.sum(want["frame"] == bad) == max_det, "the tracks outlive one frame without detections"

    trk = _tracker(max_det, 128)
    rows = torch.empty(len(want) * 2 * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for b0 in range(0, n_frames, launch):
        chunk = frames[b0:b0 + launch]
        det = np.stack([np.column_stack([d, info]).astype(np.float32) for d, info in chunk])
        cnt = [word if b0 + i == bad else len(d) for i, (d, _) in enumerate(chunk)]
        trk.run(torch.from_numpy(det).cuda(), torch.tensor(cnt, dtype=torch.int32, device="cuda"), b0, rows, count)
    torch.cuda.synchronize()
    assert trk.info()[2] == (ERR_DET_CLAMPED if flagged else 0)
    _assert_rows_equal(rows_to_numpy(rows, int(count.item())).copy(), want, f"count word {word} in frame {bad} against {clamped}")
