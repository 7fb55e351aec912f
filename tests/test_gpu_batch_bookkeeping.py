"""The batch link's bookkeeping between the search and the filter bank (csrc/batch_link.h, k_batch; DESIGN.md section 4,
round 15): the measurements that leave the filters' windows come from ONE exec region, a window that is not full reads the
ring's line of zeros; a frame's row capacity is decided once, where it is uniform; ageing and registration are one scalar
compare; `mine` is one compare of keys.

Nothing is left out of a comparison: every row of every frame of every clip is compared -- with the per-frame link and the
host ``CentroidTracker`` (test_gpu_batch_claims._all_ways) where the filter bank is off and rows must be EQUAL, with the CPU
oracle and the per-frame link where it is on -- and launches of 64, 7 and 1 frames must give the same BYTES.  Only the
row-capacity cases compare what the buffer holds, and say so.  Every clip is under 100 frames.

The ring is reached through two test hooks of the library (track.hip: ysmr_debug_ring_poison, ysmr_debug_ring_zero_line):
a fresh handle's ring positions are filled with NaN bit patterns before its first launch, so an entry that a filter bank
sums without its own track having stored it shows in the rows; and the line of zeros is read back after the runs.
"""
import ctypes

import numpy as np
import pytest

import one_barrier_clips as clips
from conftest import compare_rows
from frame_constants_clips import full_frames_clip
from link_clips import crowded_clip, oracle_rows
from test_gpu_batch_claims import (D, _all_ways, _assert_rows_equal, _bits, _f32, _field, _frame, _reference_winner, _s,
                                   _straddling_pair)
from test_gpu_batch_young import KW, _run_schedule, _same_rows, growth_frames, horizons

pytestmark = pytest.mark.gpu


def _hooks():
    from ysmr_amd import _lib
    L = _lib.lib()
    L.ysmr_debug_ring_poison.argtypes = [ctypes.c_void_p]
    L.ysmr_debug_ring_zero_line.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
    return L


def _poison(trk):
    assert _hooks().ysmr_debug_ring_poison(trk._handle) == 0


def _zero_line_words(trk):
    n = ctypes.c_longlong(-1)
    assert _hooks().ysmr_debug_ring_zero_line(trk._handle, ctypes.byref(n)) == 0
    return n.value


# ---- 1. windows that are not full ----------------------------------------------------------------------------------------
YOUNG_FRAMES = 96
# launches that END on a registration frame (30, 60, 80) and START on one (0, 31, 61, 81)
BIRTH_CUTS = (31, 30, 20, 15)


def _young():
    return crowded_clip(n_frames=YOUNG_FRAMES, n_blobs=60, seed=23)


def test_young_clip_has_the_frames_the_cases_are_about(oracle):
    """CPU: births in the first and in the last frame of a launch of BIRTH_CUTS, a filter switched on inside a launch, in
    the last frame of one (80) and in the first frame of one (81)."""
    per_frame = _young()
    ref, live, _ = oracle_rows(oracle, per_frame, use_gsff=True, n_f=3, **KW)
    first_seen = {}
    for r in ref:
        first_seen.setdefault(r[1], r[0])
    births = sorted(set(first_seen.values()))
    assert births == [0, 30, 31, 60, 61, 80, 81]
    starts = np.cumsum((0,) + BIRTH_CUTS)
    assert starts[-1] >= YOUNG_FRAMES - 1 and {0, 31, 61, 81} <= set(starts.tolist()) and {30, 60, 80} <= set((starts - 1).tolist())
    assert horizons(3) == [10, 20, 30]
    grow = {g for b in births for g in growth_frames(b, 3) if g < YOUNG_FRAMES}
    assert {80, 81} <= grow and {40, 50} <= grow          # on a launch's last and first frame, and inside one
    assert 20 < live.min() and live.max() <= 128


@pytest.mark.parametrize("n_f", [3, 2, 1])
def test_windows_that_are_not_full(oracle, n_f):
    """Handles of three, two and one filter on young tracks, every ring position poisoned with NaNs before the first launch:
    against the oracle and the per-frame link, the same bytes for launches of 64 / 7 / 1 frames and for launches cut at the
    registration frames, and the line of zeros still all zeros afterwards."""
    import torch
    from ysmr_amd.tracker import DeviceTracker
    per_frame = _young()
    ref, live, ot = oracle_rows(oracle, per_frame, use_gsff=True, shadows=2, n_f=n_f, **KW)
    cap, md = 128, 128
    base = DeviceTracker(capacity=cap, max_det=md, n_f=n_f, **KW)
    per = _run_schedule(torch, base, per_frame, [("run", 16, 1)] * YOUNG_FRAMES, md, len(ref) + 8, cap)
    compare_rows(per, ref)
    cut = {}
    for name, schedule in [(b, [("run", b, 0)] * YOUNG_FRAMES) for b in (64, 7, 1)] + [("births", [("run", b, 0) for b in BIRTH_CUTS])]:
        trk = DeviceTracker(capacity=cap, max_det=md, n_f=n_f, **KW)
        assert trk.batched
        _poison(trk)
        got = _run_schedule(torch, trk, per_frame, schedule, md, len(ref) + 8, cap)
        assert not np.isnan(got["x"]).any() and not np.isnan(got["y"]).any(), f"launches of {name}: a NaN left the ring"
        compare_rows(got, ref)
        _same_rows(got, per)
        assert trk.info()[:2] == (int(live[-1]), ot.next_id)
        assert _zero_line_words(trk) == 0, f"launches of {name}: the ring's line of zeros was written"
        cut[name] = got
    assert cut[64].tobytes() == cut[7].tobytes() == cut[1].tobytes() == cut["births"].tobytes()


# ---- 2. row capacity -----------------------------------------------------------------------------------------------------
GUARD_ROWS = 64


@pytest.mark.parametrize("short_by", ["exact", "one_row", "mid_frame"])
def test_row_capacity(oracle, short_by):
    """A row buffer that is exactly large enough, one row short (the last frame's last row), and one that ends inside
    frame 9 and stays short for the twenty frames behind it.  Compared: the rows the buffer holds, the row count (it goes
    on as if the buffer were large enough), the status word -- ERR_ROWS_CAPACITY (2) and nothing else, or 0 -- against the
    per-frame link with the same buffer, and the guard bytes behind the buffer."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker, rows_to_numpy
    frames = clips.staggered_deaths_clip(212, 30, births_at=(20,))
    _, deaths, live = clips.events(oracle, frames)
    total = int(live.sum())
    room = {"exact": total, "one_row": total - 1, "mid_frame": int(live[:9].sum()) + 50}[short_by]
    assert short_by != "mid_frame" or (live[:9].sum() < room < live[:10].sum() and deaths[8] and deaths[9])
    size = _lib.ROW_DTYPE.itemsize
    kw = dict(max_disappeared=clips.MAX_GONE, fps=30.0, use_gsff=False, capacity=768, max_det=256)

    def run(trk, batch):
        buf = torch.full(((room + GUARD_ROWS) * size,), 0xA5, dtype=torch.uint8, device="cuda")
        rows = buf[:room * size]
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        for b0 in range(0, len(frames), batch):
            chunk = frames[b0:b0 + batch]
            det = torch.zeros(len(chunk), 256, 5, dtype=torch.float32, device="cuda")
            cnt = torch.tensor([len(d) for d, _ in chunk], dtype=torch.int32, device="cuda")
            for i, (d, info) in enumerate(chunk):
                det[i, :len(d)] = torch.from_numpy(np.column_stack([d, info]).astype(np.float32)).cuda()
            trk.run(det, cnt, b0, rows, count)
        torch.cuda.synchronize()
        assert bool((buf[room * size:] == 0xA5).all()), "bytes behind the row buffer were written"
        return rows_to_numpy(rows, min(room, total)).copy(), int(count.item()), trk.info()

    one = DeviceTracker(**kw)
    one.link_mode(1)
    want, want_count, want_info = run(one, 16)
    assert want_count == total and want_info[2] == (0 if short_by == "exact" else 2)
    assert (want["frame"][-1], len(want)) == (9 if short_by == "mid_frame" else len(frames) - 1, min(room, total))
    for batch in clips.CUTS:
        trk = DeviceTracker(**kw)
        assert trk.batched
        got, count, info = run(trk, batch)
        assert (count, info) == (want_count, want_info), f"launches of {batch}"
        _assert_rows_equal(got, want, f"k_batch, launches of {batch}, against the per-frame link")


# ---- 3. ageing and deaths ------------------------------------------------------------------------------------------------
def free_wave_clip():
    """192 tracks on three waves.  From frame 1 on the 64 blobs of the SECOND wave are missing, and every fifth blob of the
    other two: all die in frame 3 -- deaths in three waves in one frame, exactly at max_disappeared -- which leaves a wave
    whose lanes are all free between two waves with tracks, and holes inside those.  Frame 6 registers seven new blobs (into
    the holes of the first wave; nobody ages), frame 7 ages again, frames 9-11 are empty (everybody ages, everybody dies in
    frame 11), frame 12 is empty on an empty table, frame 13 registers into it."""
    p = clips.lattice(192)
    stay = [q for i, q in enumerate(p) if not (64 <= i < 128) and i % 5 != 0]
    new, late = clips.lattice(7, x0=1500.0, y0=60.0), clips.lattice(40, x0=52.0, y0=900.0)
    frames = [p] + [stay] * 5 + [stay + new, stay[3:] + new, stay[3:] + new, [], [], [], [], late, late]
    return [clips._frame(q, 800 + k) for k, q in enumerate(frames)]


def test_free_wave_clip_holds_its_events(oracle):
    frames = free_wave_clip()
    births, deaths, live = clips.events(oracle, frames)
    assert {i // 64 for i in deaths[3]} == {0, 1, 2} and {i for i in range(64, 128)} <= set(deaths[3])
    assert not any(deaths[f] for f in (1, 2))                 # gone = 1, 2: nobody dies before max_disappeared is passed
    assert len(births[6]) == 7 and not deaths[6] and len(deaths[9]) == 3      # registers between frames that age
    assert live[10] > 0 and live[11] == 0 and live[12] == 0 and len(births[13]) == 40
    assert len(frames[9][0]) == 0 and len(frames[12][0]) == 0


@pytest.mark.parametrize("clip", ["free_wave", "wipe_out", "births_beside_deaths", "staggered"])
def test_ageing_and_deaths(oracle, clip):
    """Frames without detections, frames that register directly before and behind frames that age, deaths exactly at
    max_disappeared and in several waves of one frame, a free wave between two waves with tracks, an empty table at the
    start of a launch (cuts of 1) and in its middle: equal rows every way."""
    frames = {"free_wave": free_wave_clip, "wipe_out": clips.wipe_out_clip, "births_beside_deaths": clips.births_beside_deaths_clip,
              "staggered": lambda: clips.staggered_deaths_clip(212, 40, births_at=(20, 21))}[clip]()
    _, _, live = clips.events(oracle, frames)
    rows = _all_ways(frames, capacity=768, max_det=256)
    assert np.array_equal(np.bincount(rows["frame"], minlength=len(frames)), live)


# ---- 4. ties -------------------------------------------------------------------------------------------------------------
FILL = [(2400.0 + 60.0 * i, 1000.0 + 60.0 * j) for j in range(10) for i in range(15)]       # 150 stationary bystanders
E1, P1, P2 = (5000.0, 100.0), (5003.0, 100.0), (5000.0, 105.0)        # two proposals for E1, 3 px and 5 px away: no tie
E2, Q1, Q2 = (5000.0, 3000.0), (5000.0, 3006.0), (5004.0, 3000.0)     # and for E2, 6 px and 4 px: the HIGHER id is nearer
FAR = (9000.0, 9000.0)


def _wide_contest_clip(lo, hi, d, swap, extra):
    """test_gpu_batch_claims._contest_clip with the contenders in different waves of a 768-seat handle: 70 bystanders sit
    between any two of them in the table.  swap: `hi` (and `extra`) are registered later; `hi` takes seat 0, which a track
    that died left free -- the higher id in the lower seat, two waves apart -- and `extra` the first seat behind the table.
    The contest frame shows d, E1 and E2: two more columns with two proposers each, which are not ties.
    Returns (frames, contest frame, {name: id})."""
    pairs = [P1, P2, Q1, Q2]
    late = [hi] + ([extra] if extra is not None else [])
    if not swap:
        first = [lo] + FILL[:70] + [hi] + FILL[70:140] + ([extra] if extra is not None else []) + FILL[140:] + pairs
        frames = [first]
        ids = {"lo": 0, "hi": 71, "extra": 142}
        rest = FILL
    else:
        first = [FAR] + FILL[:70] + [lo] + FILL[70:] + pairs
        rest = FILL
        frames = [first] + [[lo] + rest + pairs] * 3 + [[lo] + rest + pairs + late]
        ids = {"lo": 71, "hi": len(first), "extra": len(first) + 1}
    ids.update(p1=frames[0].index(P1), p2=frames[0].index(P2), q1=frames[0].index(Q1), q2=frames[0].index(Q2))
    contest = len(frames)
    frames += [[d, E1, E2] + rest] * 2
    return [_frame(p, 900 + k) for k, p in enumerate(frames)], contest, ids


def _check_wide_contest(lo, hi, d, swap, extra=None):
    lo, hi, d = tuple(_f32(lo)), tuple(_f32(hi)), tuple(_f32(d))
    extra = None if extra is None else tuple(_f32(extra))
    per_frame, contest, ids = _wide_contest_clip(lo, hi, d, swap, extra)
    where = {ids["lo"]: lo, ids["hi"]: hi}
    if extra is not None:
        where[ids["extra"]] = extra
    winner = _reference_winner(sorted(where.items()), d)
    rows = _all_ways(per_frame, capacity=768, max_det=256)       # (and against the host tracker: its winners)
    before = rows[rows["frame"] == contest - 1]
    seat_of = {int(t): k for k, t in enumerate(before["track_id"])}
    fr = rows[rows["frame"] == contest]
    assert fr["track_id"].tolist() == sorted(fr["track_id"].tolist())
    outcome = {tid: (d if tid == winner else p, 0 if tid == winner else 1) for tid, p in where.items()}
    outcome.update({ids["p1"]: (E1, 0), ids["p2"]: (P2, 1), ids["q1"]: (Q1, 1), ids["q2"]: (E2, 0)})
    for tid, (p, gone) in outcome.items():
        r = fr[fr["track_id"] == tid]
        assert len(r) == 1 and (r["x"][0], r["y"][0], r["disappeared"][0]) == (p[0], p[1], gone), f"track {tid} in the contest frame"
    if not swap:                    # (table rows are seats while nobody has died: the contenders sit in different waves)
        seats = {t: seat_of[t] for t in where}
    else:
        # Seats are ids in frame 0 (an empty table is filled in column order) and a new track takes the lowest free seat.
        # The rows say which seats are free when `hi` (and `extra`) arrive: track 0 -- FAR, seat 0 -- is in the rows of
        # frames 0-2 and gone from frame 3 on, every other track of frame 0 is still there in frame `contest - 1`, and
        # the late ones appear in frame contest - 1 and not before.  So `hi` sits in seat 0 and `extra` behind the table.
        n0 = int(np.sum(rows["frame"] == 0))
        by_frame = [set(rows["track_id"][rows["frame"] == f].tolist()) for f in range(contest)]
        assert all(0 in by_frame[f] for f in range(3)) and all(0 not in by_frame[f] for f in range(3, contest)), "FAR did not die in frame 3"
        assert all(by_frame[f] == set(range(1, n0)) for f in range(3, contest - 1)), "another seat than 0 was freed"
        late = sorted(by_frame[contest - 1] - set(range(n0)))
        assert late == [ids["hi"]] + ([ids["extra"]] if extra is not None else []) and by_frame[contest - 1] >= set(range(1, n0))
        seats = {ids["lo"]: ids["lo"], ids["hi"]: 0}
        if extra is not None:
            seats[ids["extra"]] = n0
        assert seats[ids["hi"]] < seats[ids["lo"]] and ids["hi"] > ids["lo"]      # the higher id in the lower seat
    assert set(seats) == set(where) and len({v // 64 for v in seats.values()}) == len(where), f"contenders share a wave: {seats}"
    return winner, ids


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("case", ["equal", "same_high_bits", "straddle", "equal_roots", "third_far_below"])
def test_near_ties_between_waves_beside_columns_that_are_no_ties(case, swap):
    """The five constructions of test_gpu_batch_claims.py (their bit patterns asserted again, in numpy), capacity 768."""
    extra = None
    d = D
    if case == "equal":
        lo, hi = (D[0] - 3.0, D[1] + 4.0), (D[0] + 4.0, D[1] - 3.0)
        assert _s(lo, D) == _s(hi, D) == 25.0
        expect = "lo"
    elif case == "same_high_bits":
        lo, hi = (D[0] - 1024.0, D[1] + 2.0 ** -12), (D[0] - 1024.0, D[1])
        assert _s(hi, D) == 2.0 ** 20 and _s(lo, D) > _s(hi, D) and _field(_s(lo, D)) == _field(_s(hi, D))
        assert np.sqrt(_s(lo, D)) != np.sqrt(_s(hi, D))
        expect = "hi"
    elif case == "straddle":
        dy_small, dy_large = _straddling_pair()
        d = (1100.0, 0.5)
        lo, hi = (d[0] - 1024.0, d[1] + dy_large), (d[0] - 1024.0, d[1] - dy_small)
        s_lo, s_hi = _s(lo, d), _s(hi, d)
        assert s_lo > s_hi and _bits(s_lo) - _bits(s_hi) <= 4 and _field(s_lo) == _field(s_hi) + 1
        expect = "lo" if np.sqrt(s_lo) == np.sqrt(s_hi) else "hi"
    elif case == "equal_roots":
        lo, hi = (D[0] - 1024.0, D[1] + 2.0 ** -16), (D[0] - 1024.0, D[1])
        assert _bits(_s(lo, D)) == _bits(_s(hi, D)) + 1 and np.sqrt(_s(lo, D)) == np.sqrt(_s(hi, D)) == 1024.0
        expect = "lo"
    else:
        lo, hi, extra = (D[0] - 1024.0, D[1] + 2.0 ** -16), (D[0] - 1024.0, D[1]), (D[0] - 10.0, D[1])
        assert _field(_s(lo, D)) == _field(_s(hi, D)) and _s(extra, D) == 100.0 and _field(_s(extra, D)) + 2 < _field(_s(hi, D))
        expect = "extra"
    winner, ids = _check_wide_contest(lo, hi, d, swap, extra)
    assert winner == ids[expect]


def test_a_track_on_its_detection_beside_empty_columns():
    """s = 0: stationary blobs without a filter bank sit exactly on their detections, the smallest key there is, in columns
    nobody else proposes for -- 600 of them on ten waves, for 20 frames."""
    frames = full_frames_clip(20, 600)
    rows = _all_ways(frames, capacity=768, max_det=640)
    assert len(rows) == 20 * 600
