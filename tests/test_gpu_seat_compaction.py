"""k_batch gives up a track wave as soon as the live tracks fit without it (csrc/batch_link.h, the block at the head of the
frame loop): the tracks of the waves at and above ceil(n / 64) move into the free lanes
below, state and ring column, and the vacated waves become helpers.  Which lane holds a track decides nothing a caller
sees, so every case compares the rows of hand-made detection arrays with the CPU oracle at the batch link's tolerances
(conftest.compare_rows), in launches of 256 / 64 / 7 / 1 frames, whose rows must be the same bytes.

That the block ran (or did not) is read through two test hooks of the library (track.hip: ysmr_debug_seat_events,
ysmr_debug_track_waves) after every launch and set against ``seat_model`` below, which replays the kernel's seat policy on
the oracle's births and deaths: lowest free lane first, `n` stale by the deaths of the frame before inside a launch and
exact at its start, at most as many movers per event as the dead key table holds, the highest wave first.

The first test needs no GPU: it asserts with the model that every clip holds the events its GPU test is about.
"""
import ctypes

import numpy as np
import pytest

from conftest import compare_rows
from link_clips import oracle_rows

KW = dict(max_disappeared=2.0, fps=30.0, n_min=0, n_max=30)      # (a track unseen in three ageing frames dies in the third)
CUTS = (256, 64, 7, 1)
MOVE_WORDS = 7 * 3 + 4 + 4           # batch_link.h: BL_MOVE_WORDS, 64-bit words of a track on the move
REFRESH = 64                         # BL_REFRESH


def room_for(max_det):
    """Tracks one event moves: the key table's columns but column 0, over the words of a track."""
    return ((max_det + 3) // 4 * 4 - 1) // MOVE_WORDS


# ---- clips ---------------------------------------------------------------------------------------------------------------
def make_clip(n_blobs, n_frames, shown, seed, drift=0.05):
    """Blobs on a lattice 24 px apart that drift slowly, measured with 0.2 px of noise (float32 values); ``shown(f)``: the
    indices seen in frame f, ascending.  [(xy, info)] per frame."""
    rng = np.random.default_rng(seed)
    per_row = 40
    base = np.array([(40.0 + 24.0 * (i % per_row), 40.0 + 24.0 * (i // per_row)) for i in range(n_blobs)])
    vel = rng.normal(0, drift, base.shape)
    frames = []
    for f in range(n_frames):
        idx = np.asarray(sorted(shown(f)), int)
        xy = (base[idx] + f * vel[idx] + rng.normal(0, 0.2, (len(idx), 2))).astype(np.float32).astype(np.float64)
        info = np.column_stack([rng.uniform(1, 9, len(idx)), rng.uniform(1, 9, len(idx)), rng.uniform(0, 90, len(idx))])
        frames.append((xy.reshape(-1, 2), info.astype(np.float32).astype(np.float64)))
    return frames


def fading(n0, fades, arrivals=()):
    """shown(f) of n0 blobs from frame 0; fades: [(frame, indices)] that vanish for good from `frame` on; arrivals:
    [(frame, indices)] that appear from `frame` on."""
    def shown(f):
        s = set(range(n0))
        for at, idx in arrivals:
            if f >= at:
                s |= set(idx)
        for at, idx in fades:
            if f >= at:
                s -= set(idx)
        return s
    return shown


FADE_1 = [6 * i for i in range(20)]                                    # 20 blobs of waves 0-1
FADE_2 = [1 + 6 * i for i in range(20)] + [3 + 6 * i for i in range(5)]    # 25 more


def boundary_clip():
    """140 tracks on three waves.  20 of waves 0-1 vanish from frame 10 on and die in frame 12: 120 live tracks, wave 2's
    twelve move down.  From frame 50 on 30 new blobs: eight into the last free lanes below, 22 into wave 2.  25 more blobs
    vanish from frame 60 on: 125 live tracks, wave 2's 22 move down -- around the refresh frame 64, with every moved
    track's ring wrapped since the first move."""
    return make_clip(170, 110, fading(140, [(10, FADE_1), (60, FADE_2)], [(50, range(140, 170))]), seed=1701)


def coincidence_clip(kind):
    """40 frames of the boundary clip's first fade, shifted.  (frames, first frame number, the frame of the event in a launch
    that holds the whole clip)"""
    if kind == "after_registration":        # deaths in frame 12, three new blobs in frame 13 (123 live), the event in 14
        return make_clip(143, 40, fading(140, [(10, FADE_1)], [(13, range(140, 143))]), seed=1702), 0, 14
    if kind == "after_deaths":              # 20 die in frame 12, three more in frame 13: the event in 14 moves stale ranks
        return make_clip(140, 40, fading(140, [(10, FADE_1), (11, [1, 7, 13])]), seed=1703), 0, 14
    if kind == "before_refresh":            # the event in frame 14 is frame number 63
        return make_clip(140, 40, fading(140, [(10, FADE_1)]), seed=1704), 49, 14
    at = int(kind[3:])                      # "len19" .. : the event in the frame where the moved tracks are `at` frames old
    return make_clip(140, 40, fading(140, [(at - 4, FADE_1)]), seed=1705 + at), 0, at


COINCIDENCES = ("after_registration", "after_deaths", "before_refresh", "len19", "len20", "len29", "len30")


def twelve_waves_clip():
    """760 tracks on twelve waves; 260 scattered blobs vanish from frame 5 on (500 live: eight waves), 200 more from frame 20
    on (300: five).  An event moves at most 26 tracks: one event after the other."""
    rng = np.random.default_rng(1720)
    gone = rng.permutation(760)
    return make_clip(760, 40, fading(760, [(5, gone[:260]), (20, gone[260:460])]), seed=1721)


def small_table_clip():
    """100 tracks on two waves fading to 60, max_det 100: three tracks per event."""
    rng = np.random.default_rng(1730)
    return make_clip(100, 40, fading(100, [(5, rng.permutation(100)[:40])]), seed=1731)


def hand_over_clip():
    """The boundary clip's two fades within 70 frames: events in frame 14 and around frame 54."""
    return make_clip(170, 70, fading(140, [(10, FADE_1), (50, FADE_2)], [(40, range(140, 170))]), seed=1740)


QUIET = {      # name: (clip, capacity, max_det, use_gsff)
    "multiple_of_64": (lambda: make_clip(128, 12, fading(128, []), seed=1750), 128, 128, True),
    "within_a_wave": (lambda: make_clip(140, 16, fading(140, [(4, range(0, 140, 14))]), seed=1751), 256, 256, True),
    "empty_table": (lambda: make_clip(4, 12, lambda f: set(), seed=1752), 128, 64, True),
    "full_table": (lambda: make_clip(768, 8, fading(768, []), seed=1753), 768, 768, True),
    "no_filter_bank": (lambda: make_clip(140, 12, fading(140, []), seed=1754), 256, 256, False),
}


# ---- the seat policy, replayed ------------------------------------------------------------------------------------------
def events_of(ref):
    """(births, deaths) per frame as sorted id lists, off the oracle's rows."""
    n_frames = int(max(r[0] for r in ref)) + 1 if ref else 0
    ids = [set() for _ in range(n_frames)]
    for r in ref:
        ids[int(r[0])].add(int(r[1]))
    births = [sorted(ids[f] - (ids[f - 1] if f else set())) for f in range(n_frames)]
    deaths = [sorted((ids[f - 1] if f else set()) - ids[f]) for f in range(n_frames)]
    return births, deaths


def seat_model(births, deaths, n_frames, cut, seats, room):
    """(events per launch, tracks moved per launch, occupied waves at each launch's end, live tracks at the end)."""
    births = births + [[]] * (n_frames - len(births))
    deaths = deaths + [[]] * (n_frames - len(deaths))
    lane = {}                                   # id -> lane
    out_e, out_m, out_w = [], [], []
    for f0 in range(0, n_frames, cut):
        waves = lambda: max((v // 64 for v in lane.values()), default=-1) + 1      # noqa: E731
        helpers_from, n, ev, mv = waves(), len(lane), 0, 0
        pending = 0                             # deaths of the frame before, not yet taken off n
        for f in range(f0, min(f0 + cut, n_frames)):
            keep = (n + 63) >> 6
            if keep < helpers_from:
                movers = sorted((t for t, v in lane.items() if v >= 64 * keep), key=lambda t: (-(lane[t] // 64), lane[t]))
                taken = set(lane.values())
                free = [v for v in range(min(64 * keep, seats)) if v not in taken]
                k = min(len(movers), room)
                for t, v in zip(movers[:k], free):
                    lane[t] = v
                helpers_from = waves()
                ev, mv = ev + 1, mv + k
            n -= pending
            for t in deaths[f]:
                del lane[t]
            pending = len(deaths[f])
            if births[f]:
                taken = set(lane.values())
                free = [v for v in range(seats) if v not in taken]
                for t, v in zip(births[f], free):
                    lane[t] = v
                n += len(births[f])
                helpers_from = max(helpers_from, max(lane[t] for t in births[f]) // 64 + 1)
        out_e.append(ev); out_m.append(mv); out_w.append(waves())
    return out_e, out_m, out_w, len(lane)


def _model(oracle, frames, cut, capacity, max_det, use_gsff=True):
    ref, live, ot = oracle_rows(oracle, frames, use_gsff=use_gsff, shadows=2 if use_gsff else 0, n_f=3, **KW)
    b, d = events_of(ref)
    return ref, live, ot, seat_model(b, d, len(frames), cut, min(capacity, 768), room_for(max_det))


def test_clips_hold_their_events(oracle):
    """CPU: by the replayed policy, every clip moves tracks where its GPU test says it does."""
    ref, live, _, (ev, mv, wv, n) = _model(oracle, boundary_clip(), 256, 256, 768)
    assert (ev, mv) == ([2], [34]) and live[13] == 120 and live[-1] == 125
    births, deaths = events_of(ref)
    for cut in CUTS[1:]:
        ev, mv, wv, n = seat_model(births, deaths, 110, cut, 256, room_for(768))
        assert sum(mv) == 12 + 22 and sum(ev) >= 2 and wv[-1] == 2 == -(-n // 64)
    for kind in COINCIDENCES:
        frames, first, at = coincidence_clip(kind)
        ref, live, _, (ev, mv, wv, n) = _model(oracle, frames, 256, 256, 768)
        b, d = events_of(ref)
        assert (ev, mv) == ([1], [12]) and wv[-1] == 2 == -(-n // 64), kind
        # the event's frame: the first whose head sees n <= 128 (live tracks behind the frame before, plus its deaths)
        heads = [f for f in range(1, 40) if live[f - 1] + len(d[f - 1]) <= 128]
        assert heads[0] == at, (kind, heads[0])
        if kind == "after_registration":
            assert len(b[at - 1]) == 3
        if kind == "after_deaths":
            assert len(d[at - 1]) == 3 and len(d[at - 2]) == 20
        if kind == "before_refresh":
            assert (first + at + 1) % REFRESH == 0
    _, live, _, (ev, mv, wv, n) = _model(oracle, twelve_waves_clip(), 256, 768, 768)
    assert live[0] == 760 and live[-1] == 300 and ev[0] >= 8 and mv[0] > 150 and wv[-1] == 5
    _, live, _, (ev, mv, wv, n) = _model(oracle, small_table_clip(), 256, 128, 100)
    assert room_for(100) == 3 and live[-1] == 60 and ev[0] >= 5 and mv[0] > 3 * (ev[0] - 1) and wv[-1] == 1
    for name, (clip, cap, md, gsff) in QUIET.items():
        _, live, _, (ev, mv, wv, n) = _model(oracle, clip(), 256, cap, md, gsff)
        assert (ev, mv) == ([0], [0]) and wv[-1] == -(-n // 64), name
    _, live, _, (ev, mv, _, _) = _model(oracle, hand_over_clip(), 256, 256, 768)
    assert mv == [34]


# ---- the GPU side -------------------------------------------------------------------------------------------------------
def _hooks():
    from ysmr_amd import _lib
    L = _lib.lib()
    L.ysmr_debug_ring_poison.argtypes = [ctypes.c_void_p]
    L.ysmr_debug_seat_events.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.ysmr_debug_track_waves.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    return L


def _seat_words(trk):
    e, m, w = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert _hooks().ysmr_debug_seat_events(trk._handle, ctypes.byref(e), ctypes.byref(m)) == 0
    assert _hooks().ysmr_debug_track_waves(trk._handle, ctypes.byref(w)) == 0
    return e.value, m.value, w.value


def _upload(torch, chunk, max_det):
    det = np.zeros((len(chunk), max_det, 5), np.float32)
    for i, (d, info) in enumerate(chunk):
        det[i, :len(d)] = np.column_stack([d, info])
    return torch.from_numpy(det).cuda(), torch.tensor([len(d) for d, _ in chunk], dtype=torch.int32, device="cuda")


def _launches(torch, trk, frames, cut, max_det, rows, count, first=0, f_from=0, f_to=None):
    """Frames [f_from, f_to) in launches of `cut`; the seat words after every launch."""
    words = []
    f_to = len(frames) if f_to is None else f_to
    for f0 in range(f_from, f_to, cut):
        det, cnt = _upload(torch, frames[f0:min(f0 + cut, f_to)], max_det)
        trk.run(det, cnt, first + f0, rows, count)
        words.append(_seat_words(trk))
    return words


def _check_clip(oracle, frames, capacity, max_det, first=0, use_gsff=True, poison=False, cuts=CUTS):
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker, rows_to_numpy
    ref, live, ot = oracle_rows(oracle, frames, use_gsff=use_gsff, shadows=2 if use_gsff else 0, n_f=3, **KW)
    ref = [(r[0] + first,) + tuple(r[1:]) for r in ref]
    b, d = events_of([(r[0] - first,) + tuple(r[1:]) for r in ref])
    seen = {}
    for cut in cuts:
        trk = DeviceTracker(capacity=capacity, max_det=max_det, n_f=3, use_gsff=use_gsff, **KW)
        assert trk.batched
        if poison:
            assert _hooks().ysmr_debug_ring_poison(trk._handle) == 0
        rows = torch.empty((len(ref) + 8) * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        words = _launches(torch, trk, frames, cut, max_det, rows, count, first)
        torch.cuda.synchronize()
        assert trk.info() == (int(live[-1]), ot.next_id, 0)
        got = rows_to_numpy(rows, int(count.item())).copy()
        assert not np.isnan(got["x"]).any() and not np.isnan(got["y"]).any(), f"launches of {cut}: a NaN left the ring"
        compare_rows(got, ref)
        ev, mv, wv, n = seat_model(b, d, len(frames), cut, min(capacity, 768), room_for(max_det))
        assert [w[0] for w in words] == ev, f"launches of {cut}: events per launch"
        assert [w[1] for w in words] == mv, f"launches of {cut}: tracks moved per launch"
        assert [w[2] for w in words] == wv, f"launches of {cut}: occupied waves at the end of each launch"
        assert words[-1][2] == -(-n // 64), f"launches of {cut}: {words[-1][2]} waves hold {n} tracks"
        seen[cut] = (got, sum(ev), sum(mv), trk)
    first_cut = seen[cuts[0]][0]
    for cut in cuts[1:]:
        assert seen[cut][0].tobytes() == first_cut.tobytes(), f"launches of {cut} and of {cuts[0]} frames give different rows"
    return seen, ref, ot


@pytest.mark.gpu
def test_across_one_wave_boundary(oracle):
    seen, _, _ = _check_clip(oracle, boundary_clip(), 256, 768, poison=True)
    assert seen[256][1:3] == (2, 34)
    assert all(s[2] == 34 for s in seen.values())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", COINCIDENCES)
def test_events_beside_the_other_rare_frames(oracle, kind):
    frames, first, _ = coincidence_clip(kind)
    seen, _, _ = _check_clip(oracle, frames, 256, 768, first=first, poison=True)
    assert seen[256][1:3] == (1, 12)


@pytest.mark.gpu
def test_twelve_waves_down_to_five(oracle):
    seen, _, _ = _check_clip(oracle, twelve_waves_clip(), 768, 768)
    assert seen[256][1] >= 8 and seen[256][2] > 150


@pytest.mark.gpu
@pytest.mark.parametrize("use_gsff", [True, False])
def test_the_table_does_not_hold_all_movers(oracle, use_gsff):
    seen, _, _ = _check_clip(oracle, small_table_clip(), 128, 100, use_gsff=use_gsff)
    assert seen[256][1] >= 5 and seen[256][2] > 3 * (seen[256][1] - 1)


def _check_peek(trk, ot, use_gsff=True):
    """ids and `disappeared` exactly; the positions the oracle determines (conftest.compare_rows) to 1e-9."""
    from oracle.ysmr_oracle import OracleTracker
    ids, xy, gone = trk.peek()
    assert list(ids) == [t.tid for t in ot.tracks] and list(gone) == [t.gone for t in ot.tracks]
    want = np.array([t.pos for t in ot.tracks], float).reshape(-1, 2)
    firm = np.asarray(ot.last_sens) <= OracleTracker.ILL_CONDITIONED if use_gsff and len(ot.tracks) else np.ones(len(want), bool)
    np.testing.assert_allclose(xy[firm], want[firm], rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(QUIET))
def test_nothing_to_do(oracle, name):
    clip, cap, md, gsff = QUIET[name]
    seen, _, ot = _check_clip(oracle, clip(), cap, md, use_gsff=gsff)
    for cut, (_, ev, mv, trk) in seen.items():
        assert (ev, mv) == (0, 0), f"launches of {cut}"
        _check_peek(trk, ot, gsff)


@pytest.mark.gpu
def test_state_hand_over(oracle):
    """A launch with an event, the peek, twenty frames through update() (the per-frame layout: k_to_std), a batch launch
    again (k_to_batch) with the second event."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker, rows_to_numpy
    frames = hand_over_clip()
    kw = dict(use_gsff=True, shadows=2, n_f=3, **KW)
    ref, live, ot_end = oracle_rows(oracle, frames, **kw)
    _, _, ot_20 = oracle_rows(oracle, frames[:20], **kw)
    cap, md = 256, 768       # (max_det 768: the key table holds 26 movers, an event moves a whole wave's)
    trk = DeviceTracker(capacity=cap, max_det=md, n_f=3, **KW)
    # (no ring poison here: k_to_std hands the per-frame link all of a ring column, and that link multiplies the entries
    # beyond a young track's history by gains of zero -- zeros in a fresh handle, NaNs in a poisoned one)
    size = _lib.ROW_DTYPE.itemsize
    rows = torch.empty((len(ref) + 8) * size, dtype=torch.uint8, device="cuda")
    one = torch.empty(cap * size, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    n_one = torch.zeros(1, dtype=torch.int32, device="cuda")
    words = _launches(torch, trk, frames, 20, md, rows, count, f_to=20)
    assert words == [(1, 12, 2)]
    _check_peek(trk, ot_20)
    pieces = [rows_to_numpy(rows, int(count.item())).copy()]
    for f in range(20, 40):
        xy, info = frames[f]
        dd = torch.from_numpy(np.column_stack([xy, info]).astype(np.float32)).cuda()
        trk.update(dd, m=len(xy), frame=f, rows=one, n_rows=n_one)
        pieces.append(rows_to_numpy(one, int(n_one.item())).copy())
    count.zero_()
    words = _launches(torch, trk, frames, 256, md, rows, count, f_from=40)
    torch.cuda.synchronize()
    pieces.append(rows_to_numpy(rows, int(count.item())).copy())
    assert words[0][1] == 22 and words[0][2] == 2
    assert trk.info() == (int(live[-1]), ot_end.next_id, 0)
    compare_rows(np.concatenate(pieces), ref)
    _check_peek(trk, ot_end)
