"""The batch link on YOUNG tracks: the frames in which a track's filter bank leaves its steady path (batch_link.h,
bl_gsff<GATED>: the seeding of a new track, a filter switched on when the history reaches its horizon) and the frames
around them, in which the ring entries that leave the windows are requested for some filters and not for others.

k_batch carries, per lane, the history length at which the next of these happens instead of the filter mode; the value is
not stored between launches but derived from the stored mode and turned back into it.  So the clips here put such frames
where that matters: on the first and on the last frame of a launch, on the frame whose number is a multiple of 64 (the
window sums are re-summed from the ring), on tracks of different ages inside one wave, and right behind a change of the
table's layout.  Everything is compared with the oracle and with the per-frame link (k_frame), as
tests/test_gpu_batch_link.py does: ids, counters and row order exact, positions to 1e-9; and the rows of one clip must be
the same BYTES however its frames are cut into launches (64 / 7 / 1).

A live lane never reaches the filter bank with an empty history unless its track was born in that frame: every kernel that
registers a track (k_batch, k_frame, k_link + k_track, k_track_lanes) runs the filter bank on it in the same frame, which
leaves n_i[0] >= 1 entries.  The schedules below that switch the layout or call update() directly behind a registration
frame are the check: a seat that arrived with length 0 and a mode would be seeded a second time there.
"""
import numpy as np
import pytest

from conftest import compare_rows
from link_clips import crowded_clip, oracle_rows

RTOL = ATOL = 1e-9
KW = dict(max_disappeared=5.0, fps=30.0, n_min=0, n_max=30)
# crowded_clip's frames that show new blobs (link_clips.py: `full`); tracks are registered there and in frame 0
BIRTH_FRAMES = (0, 30, 31, 60, 61, 80, 81, 104)


def young_clip():
    """link_clips.crowded_clip with few blobs: ~60-110 live tracks in two waves, born in eight different frames (seats
    freed by the deaths in between are taken again, so ages mix inside a wave)."""
    return crowded_clip(n_frames=112, n_blobs=60, seed=23)


def horizons(n_f, n_min=0, n_max=30):
    """ysmr_tracker_create's n_i (gsff.py: int(n_min + p * i), p = (n_max - n_min) / n_f)."""
    p = (n_max - n_min) / n_f
    return [int(n_min + p * i) for i in range(1, n_f + 1)]


def growth_frames(birth, n_f):
    """Frames in which a track born in `birth` switches a filter on: its history starts with n_i[0] entries in the birth
    frame (filter 0 on at once) and gains one per frame."""
    n = horizons(n_f)
    return [birth + (h - n[0]) for h in n[1:]]


def test_young_clip_puts_the_rare_frames_where_the_test_needs_them(oracle):
    """CPU: the clip's births are where BIRTH_FRAMES says, and with three filters (horizons 10, 20, 30) a filter is
    switched on in the first frame of a launch of 7, in the last frame of one, and young tracks meet frame 64."""
    per_frame = young_clip()
    ref, live, ot = oracle_rows(oracle, per_frame, use_gsff=True, n_f=3, **KW)
    first_seen = {}
    for r in ref:
        first_seen.setdefault(r[1], r[0])
    births = sorted(set(first_seen.values()))
    assert births == list(BIRTH_FRAMES)
    assert horizons(3) == [10, 20, 30] and horizons(2) == [15, 30] and horizons(1) == [30]
    grow = sorted({g for b in births for g in growth_frames(b, 3) if g < len(per_frame)})
    assert any(g % 7 == 0 for g in grow) and any(g % 7 == 6 for g in grow)           # first / last frame of a launch of 7
    assert any(g % 64 == 0 for g in grow) or any(b < 64 < b + 20 for b in births)    # frame 64 on a track not yet grown
    assert 64 < live.max() <= 128 and live.min() > 20                                # two waves, never empty
    # tracks of at least three ages alive at once in the first wave's worth of table rows at frame 64
    at64 = [first_seen[r[1]] for r in ref if r[0] == 64][:64]
    assert len(set(at64)) >= 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _upload(torch, chunk, max_det):
    det = torch.zeros(len(chunk), max_det, 5, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(len(chunk), dtype=torch.int32, device="cuda")
    for i, (d, info) in enumerate(chunk):
        if len(d):
            det[i, :len(d)] = torch.from_numpy(np.column_stack([d, info]).astype(np.float32)).cuda()
        cnt[i] = len(d)
    return det, cnt


def _run_schedule(torch, trk, per_frame, schedule, max_det, rows_cap, capacity):
    """schedule: [("run", n_frames, link_mode) | ("update",)] -- launches of n_frames frames with the table in the batch
    (0) or per-frame (1) layout, and single-frame update() calls; returns the clip's rows in order."""
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    rows = torch.empty(rows_cap * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    one = torch.empty(capacity * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    n_one = torch.zeros(1, dtype=torch.int32, device="cuda")
    pieces, f = [], 0
    for step in schedule:
        if f >= len(per_frame):
            break
        if step[0] == "run":
            nb = min(step[1], len(per_frame) - f)
            det, cnt = _upload(torch, per_frame[f:f + nb], max_det)
            trk.link_mode(step[2])
            count.zero_()
            trk.run(det, cnt, f, rows, count)
            pieces.append(rows_to_numpy(rows, int(count.item())).copy())
            f += nb
        else:
            xy, info = per_frame[f]
            dd = torch.from_numpy(np.column_stack([xy, info]).astype(np.float32)).cuda()
            trk.update(dd, m=len(xy), frame=f, rows=one, n_rows=n_one)
            pieces.append(rows_to_numpy(one, int(n_one.item())).copy())
            f += 1
    assert f == len(per_frame), "the schedule does not cover the clip"
    torch.cuda.synchronize()
    assert trk.info()[2] == 0
    return np.concatenate(pieces)


def _same_rows(a, b):
    for key in ("frame", "track_id", "disappeared", "w", "h", "angle"):
        np.testing.assert_array_equal(a[key], b[key])
    np.testing.assert_allclose(a["x"], b["x"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a["y"], b["y"], rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("n_f", [3, 2, 1])
def test_young_tracks_across_batch_cuts(torch_cuda, oracle, n_f):
    """Launches of 64, 7 and 1 frames, handles of three, two and one filter: against the oracle and the per-frame link, and
    the same bytes for every cut.  Cuts of 7 put a filter's first frame on a launch's first frame (frame 70, 91: the
    threshold comes out of the stored mode) and on its last (20, 41, 90: it goes back into it); cuts of 1 do both in every
    frame; frame 64 re-sums the windows of tracks born in frames 60 and 61, whose longer windows are not full."""
    from ysmr_amd.tracker import DeviceTracker
    per_frame = young_clip()
    ref, live, ot = oracle_rows(oracle, per_frame, use_gsff=True, shadows=2, n_f=n_f, **KW)
    cap, md = 128, 128
    n_all = len(per_frame)
    base = DeviceTracker(capacity=cap, max_det=md, n_f=n_f, **KW)
    assert not base.fused or base.batched
    per = _run_schedule(torch_cuda, base, per_frame, [("run", 16, 1)] * n_all, md, len(ref) + 8, cap)      # k_frame
    compare_rows(per, ref)
    cut = {}
    for batch in (64, 7, 1):
        trk = DeviceTracker(capacity=cap, max_det=md, n_f=n_f, **KW)
        assert trk.batched
        got = _run_schedule(torch_cuda, trk, per_frame, [("run", batch, 0)] * n_all, md, len(ref) + 8, cap)
        compare_rows(got, ref)
        _same_rows(got, per)
        assert trk.info()[:2] == (int(live[-1]), ot.next_id)
        cut[batch] = got
    assert cut[64].tobytes() == cut[7].tobytes() == cut[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_f", [3, 2])
def test_layout_switch_and_update_right_behind_a_registration(torch_cuda, oracle, n_f):
    """The table changes its layout (k_to_std / k_to_batch) with tracks in it that were registered in the frame before:
    a launch that ENDS on a registration frame (30, 60, 80), then the per-frame link, an update() call, or another batch
    launch; and update() calls ON registration frames (31, 61, 81) with a batch launch right behind them."""
    from ysmr_amd.tracker import DeviceTracker
    per_frame = young_clip()
    ref, live, ot = oracle_rows(oracle, per_frame, use_gsff=True, shadows=2, n_f=n_f, **KW)
    cap, md = 128, 128
    schedules = {
        # frames 0..30 | per-frame link 31..40 | batch 41..60 | update 61 | batch 62..80 | update 81 | per-frame | batch
        "switch": [("run", 31, 0), ("run", 10, 1), ("run", 20, 0), ("update",), ("run", 19, 0), ("update",), ("run", 9, 1), ("run", 64, 0)],
        # a launch of one frame per registration frame, the other layout right behind it
        "single": [("run", 1, 0), ("run", 29, 1), ("run", 1, 0), ("run", 1, 1), ("run", 28, 0), ("run", 1, 1), ("run", 1, 0),
                   ("update",), ("run", 18, 0), ("run", 1, 0), ("update",), ("update",), ("run", 64, 0)],
    }
    for name, schedule in schedules.items():
        trk = DeviceTracker(capacity=cap, max_det=md, n_f=n_f, **KW)
        got = _run_schedule(torch_cuda, trk, per_frame, schedule, md, len(ref) + 8, cap)
        compare_rows(got, ref)
        assert trk.info()[:2] == (int(live[-1]), ot.next_id), name
