"""The batch link with ONE workgroup barrier per frame (csrc/batch_link.h, k_batch, above the frame loop): the ranks, the
row and the counts of a frame are written behind the NEXT frame's barrier A -- the last frame's behind a barrier after the
loop -- the claim key carries a rank that the last frame's deaths have not been taken off yet, three key tables rotate,
and the deaths are counted in running counts that are never reset.

Every clip (tests/one_barrier_clips.py: stationary blobs, no filter bank, so every link must give EQUAL rows) runs through
k_batch in launches of 64 / 7 / 1 frames, through the per-frame link and through the host ``CentroidTracker``
(test_gpu_batch_claims._all_ways).  Before that the CPU oracle says that the clip holds the event the test is named for.

The cap on what is compared: none.  Every row of every frame of a clip is compared; the row buffers are sized for all of
them (``_run``), and ``_all_ways`` ends with ``at == len(rows)``.  Only the test of a full row buffer compares less -- the
rows the buffer holds -- and says so.
"""
import numpy as np
import pytest

import one_barrier_clips as clips
from test_gpu_batch_claims import _all_ways, _assert_rows_equal, _run, _s

pytestmark = pytest.mark.gpu


def _frames_with(per_frame_lists):
    return [f for f, x in enumerate(per_frame_lists) if len(x)]


def test_deaths_in_consecutive_frames_across_every_launch_cut(oracle):
    """212 tracks on four waves; from frame 5 to frame 68 every ageing frame deregisters three tracks, one per wave of
    three; frames 20 and 41 register sixteen tracks in between (and age nobody).  Launches of 7 frames end with frame 6
    and start with frame 7, launches of 64 end with frame 63 and start with frame 64: deaths in all four."""
    frames = clips.staggered_deaths_clip(212, 72, births_at=(20, 41))
    births, deaths, live = clips.events(oracle, frames)
    dying = _frames_with(deaths)
    assert set(range(5, 69)) - {20, 41} <= set(dying)
    assert all(len(deaths[f]) >= 3 for f in dying)
    for f in (6, 7, 63, 64):                                    # last / first frame of a launch of 7 and of 64
        assert len({i // 64 for i in deaths[f]}) == 3, "the frame's deaths sit in three different waves"
    assert _frames_with(births) == [0, 20, 41] and not deaths[20] and not deaths[41]
    rows = _all_ways(frames, capacity=768, max_det=256)
    assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)
    _all_ways(frames, capacity=256, max_det=256)


def test_every_track_dies_in_one_frame_then_empty_then_registration(oracle):
    frames = clips.wipe_out_clip()
    births, deaths, live = clips.events(oracle, frames)
    assert len(deaths[3]) == 40 and live[3] == 0
    assert len(frames[4][0]) == 0 and live[4] == 0              # an empty frame on an empty table
    assert len(births[5]) == 30 and live[5] == 30
    assert len(deaths[11]) == 5
    for cap in (128, 768):
        rows = _all_ways(frames, capacity=cap, max_det=64)
        assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)


def test_registration_right_behind_a_death_frame_and_the_reverse(oracle):
    frames = clips.births_beside_deaths_clip()
    births, deaths, live = clips.events(oracle, frames)
    assert deaths[3] and births[4] and not deaths[4]            # a registration frame right behind a death frame
    assert births[7] and deaths[8] and not births[8]            # a death frame right behind a registration frame
    for cap in (128, 768):
        rows = _all_ways(frames, capacity=cap, max_det=64)
        assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)


def test_exact_tie_in_the_frame_after_older_tracks_died(oracle):
    """The contest frame's claim key is built from ranks that are stale by the three deaths of the frame before; the
    lower id sits in the higher seat.  The tie goes to the lower id."""
    frames, contest, lo, hi, d = clips.stale_rank_contest_clip()
    assert _s(lo, d) == _s(hi, d) == 25.0
    births, deaths, live = clips.events(oracle, frames)
    assert deaths[3] == [3] and births[4] == [30]               # `far` leaves seat 3, `hi` takes it with id 30
    assert deaths[contest - 1] == [0, 1, 2] and not deaths[contest]      # ids below lo's: its rank is stale by three
    for cap in (128, 768):
        rows = _all_ways(frames, capacity=cap, max_det=64)
        fr = rows[rows["frame"] == contest]
        assert fr["track_id"].tolist() == sorted(fr["track_id"].tolist())
        won, lost = fr[fr["track_id"] == 4], fr[fr["track_id"] == 30]
        assert (won["x"][0], won["y"][0], won["disappeared"][0]) == (d[0], d[1], 0)
        assert (lost["x"][0], lost["y"][0], lost["disappeared"][0]) == (hi[0], hi[1], 1)


def test_exact_claim_path_in_a_frame_that_registers(oracle):
    frames, at, lo, hi, d = clips.tie_in_a_registration_frame_clip()
    assert _s(lo, d) == _s(hi, d) == 25.0                       # equal keys: the frame takes the exact claim path
    births, deaths, live = clips.events(oracle, frames)
    assert len(frames[at][0]) > live[at - 1] and len(births[at]) == 5
    for cap in (128, 768):
        rows = _all_ways(frames, capacity=cap, max_det=64)
        fr = rows[rows["frame"] == at]
        won, lost = fr[fr["track_id"] == 0], fr[fr["track_id"] == 1]
        assert (won["x"][0], won["y"][0]) == d
        assert (lost["x"][0], lost["y"][0], lost["disappeared"][0]) == (hi[0], hi[1], 0)      # (nobody is aged in such a frame)


def test_all_twelve_waves_seated(oracle):
    """More than 704 live tracks throughout: no helper waves, the track waves request the grid blocks and clear the key
    tables themselves.  Deaths in consecutive frames, four per frame in four waves, and a registration among them."""
    frames = clips.staggered_deaths_clip(740, 18, per_frame=4, stride=180, births_at=(12,))
    births, deaths, live = clips.events(oracle, frames)
    assert live.min() > 704 and live.max() <= 768
    assert set(range(5, 18)) - {12} <= set(_frames_with(deaths)) and len(births[12]) == 20
    assert len({i // 64 for i in deaths[6]}) == 4
    rows = _all_ways(frames, capacity=768, max_det=1024)
    assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)


def test_row_buffer_full_in_the_middle_of_a_launch(oracle):
    """A row buffer that ends inside frame 9 of the clip, in the middle of every launch of 64 and of 7 frames: the error bit
    is raised, the count goes on as if the buffer were large enough, and the rows the buffer holds -- all that is compared
    here -- are those of the per-frame link with the same buffer."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker, rows_to_numpy
    frames = clips.staggered_deaths_clip(212, 30, births_at=(20,))
    _, deaths, live = clips.events(oracle, frames)
    room = int(live[:9].sum()) + 50
    assert live[:9].sum() < room < live[:10].sum() and deaths[8] and deaths[9]
    kw = dict(max_disappeared=clips.MAX_GONE, fps=30.0, use_gsff=False, capacity=768, max_det=256)

    def run(trk, batch):
        rows = torch.zeros(room * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        for b0 in range(0, len(frames), batch):
            chunk = frames[b0:b0 + batch]
            det = torch.zeros(len(chunk), 256, 5, dtype=torch.float32, device="cuda")
            cnt = torch.tensor([len(d) for d, _ in chunk], dtype=torch.int32, device="cuda")
            for i, (d, info) in enumerate(chunk):
                det[i, :len(d)] = torch.from_numpy(np.column_stack([d, info]).astype(np.float32)).cuda()
            trk.run(det, cnt, b0, rows, count)
        torch.cuda.synchronize()
        return rows_to_numpy(rows, room).copy(), int(count.item()), trk.info()

    one = DeviceTracker(**kw)
    one.link_mode(1)
    want, want_count, want_info = run(one, 16)
    assert want_count == live.sum() and want_info[2] == 2       # ERR_ROWS_CAPACITY, and nothing else
    for batch in clips.CUTS:
        trk = DeviceTracker(**kw)
        assert trk.batched
        got, count, info = run(trk, batch)
        assert (count, info) == (want_count, want_info)
        _assert_rows_equal(got, want, f"k_batch, launches of {batch}, against the per-frame link")


def test_largest_detection_tables_still_link_in_one_launch(oracle):
    """max_det = 2456 is the largest table the batch link serves: with a third key table its LDS still fits."""
    from ysmr_amd.tracker import DeviceTracker
    trk = DeviceTracker(max_disappeared=clips.MAX_GONE, fps=30.0, use_gsff=False, capacity=768, max_det=2456)
    assert trk.batched
    frames = clips.births_beside_deaths_clip()
    _, _, live = clips.events(oracle, frames)
    rows = _all_ways(frames, capacity=768, max_det=2456)
    assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)


def test_filter_bank_on_deaths_and_births_in_every_cut(oracle):
    """The same with the filter bank on and moving blobs: launches of 64 / 7 / 1 frames give identical rows, the per-frame
    link the same ids, counters and row order (positions to 1e-9: its filter bank sums in another order)."""
    from link_clips import crowded_clip
    from ysmr_amd.tracker import DeviceTracker
    frames = crowded_clip(n_frames=80, n_blobs=400, seed=33)
    kw = dict(max_disappeared=5.0, fps=30.0, n_min=0, n_max=30, n_f=3, capacity=768, max_det=1024)
    rows = None
    for batch in clips.CUTS:
        trk = DeviceTracker(**kw)
        assert trk.batched
        got = _run(trk, frames, batch, 1024)
        rows = got if rows is None else rows
        _assert_rows_equal(got, rows, f"k_batch, launches of {batch} against 64")
    per_frame = np.bincount(rows["frame"], minlength=len(frames))
    assert (np.diff(per_frame) < 0).any() and (np.diff(per_frame) > 0).any()      # deaths and births
    one = DeviceTracker(**kw)
    one.link_mode(1)
    _assert_rows_equal(_run(one, frames, 16, 1024), rows, "per-frame link against k_batch", xy_tol=1e-9)
