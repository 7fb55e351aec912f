"""The refresh of the window sums from the ring (csrc/batch_link.h, bl_sums_from_ring<true>): in every frame whose NUMBER
is a multiple of 64 k_batch sums each live track's history again, entry by entry in the order of the entries' ages.  The
entries are requested in groups (BL_RING_GROUP) as far as the handle's largest horizon; a lane asks for entries beyond its
own history, and the last group for ages beyond the horizon, and neither may reach a sum.

What the clip holds is asserted on the oracle first (CPU).  The history of a track starts as n_i[0] copies of its first
measurement (gsff.py:281) and gains one entry per frame, so with the default horizons (10, 20, 30) no history is shorter
than 11 where a refresh meets it; the classes below 10 are met by a handle with the horizons (4, 8, 13), SHORT -- whose
largest horizon is also no multiple of the group, so that its last group asks for ages beyond it.

The recording tests/golden/ring_refresh_rows.npz holds the rows of frames 64..85 and 128..133 (RECORDED: no earlier frame
refreshes anything, frame 0 has no track; a sum that the refresh of frame 64 records for a filter that is not switched on
yet is first used when the history reaches that filter's horizon, 21 frames later at the most) of the clip in launches of 64
frames, for the handles of HANDLES, as the library of the commit BEFORE the grouped refresh (one entry per round trip, 31 of
them) wrote them on an MI355X:
    YSMR_HIP_LIB=<that commit's libysmr_hip.so> python tests/test_gpu_ring_refresh.py <output.npz>
Rows of the oracle agree with it to 1e-9 only; a sum taken in another order, or an entry too many, differs from the
recording in its last bits, and only from the recording: every schedule of one build runs the same refresh.
"""
import os
import sys

import numpy as np
import pytest

from conftest import compare_rows, golden
from link_clips import _f32, _info, oracle_rows
from test_gpu_batch_young import KW, _upload, horizons

N_FRAMES = 134
REFRESH = (64, 128)
CAP = MD = 128
# frames that show every blob and four new ones (a frame registers tracks only when it holds more detections than there are
# tracks): in the refresh frames themselves, in the frame before, and 2-6, 6-14, 14-20 and more than 32 frames before them
BIRTH_FRAMES = (0, 20, 44, 50, 58, 63, 64, 90, 108, 114, 122, 127, 128)
LEAVE_FRAMES = {30: 6, 61: 3, 125: 3}      # blobs that leave for good: their tracks are lost at the next refresh, and die later
SHORT = dict(max_disappeared=5.0, fps=30.0, n_min=0, n_max=13)       # horizons (4, 8, 13)
HANDLES = {"nf3": (KW, 3), "nf2": (KW, 2), "nf1": (KW, 1), "short": (SHORT, 3)}
GOLDEN = "ring_refresh_rows.npz"


def _recorded(rows):
    """The rows of the frames the recording holds."""
    f = rows["frame"]
    return rows[((f >= 64) & (f < 86)) | (f >= 128)]


def refresh_clip():
    rng = np.random.default_rng(41)
    n0 = 66
    pos = np.column_stack([rng.uniform(10, 1218, n0), rng.uniform(10, 912, n0)])
    vel = rng.normal(0, 0.8, (n0, 2))
    alive = np.ones(n0, bool)
    frames = []
    for f in range(N_FRAMES):
        pos = pos + vel + rng.normal(0, 0.15, pos.shape)
        if f in LEAVE_FRAMES:
            alive[rng.choice(np.nonzero(alive)[0], LEAVE_FRAMES[f], replace=False)] = False
        full = f in BIRTH_FRAMES
        keep = alive & (np.ones(len(pos), bool) if full else rng.random(len(pos)) > 0.03)
        xy = pos[keep]
        if full and f:
            fresh = np.column_stack([rng.uniform(10, 1218, 4), rng.uniform(10, 912, 4)])
            pos = np.vstack([pos, fresh]); vel = np.vstack([vel, rng.normal(0, 0.8, (4, 2))])
            alive = np.concatenate([alive, np.ones(4, bool)])
            xy = np.vstack([xy, fresh])
        xy = _f32(xy)
        frames.append((xy, _f32(_info(rng, len(xy)))))
    return frames


STATIONARY_FRAMES, STATIONARY_FIRST = 40, 30


def stationary_clip():
    """600 lattice points seen in every one of 40 frames, numbered from 30: nine full waves, 24 live lanes beside 40 dead ones
    in the tenth, two helper waves, when frame 64 -- the clip's frame 34 -- refreshes histories of 44 entries."""
    from frame_constants_clips import full_frames_clip
    return full_frames_clip(STATIONARY_FRAMES, 600)


_REF = {}


def _oracle(oracle, name, shadows=2):
    """The clip through the oracle, once per handle."""
    if name not in _REF:
        kw, n_f = HANDLES[name]
        _REF[name] = oracle_rows(oracle, refresh_clip(), use_gsff=True, shadows=shadows, n_f=n_f, **kw)
    return _REF[name]


def _first_seen(ref):
    first = {}
    for r in ref:
        first.setdefault(r[1], r[0])
    return first


def test_the_clip_holds_what_the_cases_are_about(oracle):
    """CPU.  At both refresh frames: live tracks whose history (n_i[0] + frames since the birth, before the frame) is
    10..19, 20..29 and 32 or more entries long with the default horizons, and 1..9 long with the short ones; a track born in
    the frame before and tracks born in the refresh frame itself; a track that was lost in the frame before (a zero box,
    tracker.py): what it stored in the ring there is its own prediction, a full double, where a measurement is a float32
    centre; 60-110 tracks, in two waves at the refreshes."""
    assert horizons(3) == [10, 20, 30] and horizons(2) == [15, 30] and horizons(1) == [30]
    assert horizons(3, SHORT["n_min"], SHORT["n_max"]) == [4, 8, 13]
    for name, n0 in (("nf3", 10), ("short", 4)):
        ref, live, _ = _oracle(oracle, name)
        first = _first_seen(ref)
        assert sorted(set(first.values())) == list(BIRTH_FRAMES), name
        assert 60 <= live.min() and live.max() <= 110 and all(live[F] > 64 for F in REFRESH), name
        for F in REFRESH:
            ids = [r[1] for r in ref if r[0] == F]
            length = {i: n0 + (F - first[i]) for i in ids if first[i] < F}
            have = set(length.values())
            if name == "nf3":
                assert have & set(range(10, 20)) and have & set(range(20, 30)) and any(v >= 32 for v in have), (F, sorted(have))
            else:
                assert have & set(range(1, 10)) and any(v >= 32 for v in have), (F, sorted(have))
            assert any(first[i] == F - 1 for i in ids) and any(first[i] == F for i in ids), F
            # (a track without a detection carries a zero box, tracker.py; its position is its filter bank's prediction)
            lost = [r for r in ref if r[0] == F - 1 and r[4] == 0.0 and r[5] == 0.0 and first[r[1]] < F - 1 and r[1] in ids]
            assert lost, F


def _cuts(n, r):
    """Launch lengths for a clip of n frames: 64 / 7 / 1, and the refresh frame (clip index r) as a launch's first, last and
    an inner (fourth) frame."""
    def upto(p):      # launches of at most 64 frames that end in front of clip index p
        return ([p - 64] if p > 64 else []) + [min(p, 64)]
    return {"64": [64] * n, "7": [7] * n, "1": [1] * n, "first": upto(r) + [64] * n, "last": upto(r + 1) + [64] * n,
            "inner": upto(r - 3) + [64] * n}


def _run(torch, name, per_frame, lengths, first=0, poison=False, cap=CAP, md=MD, rows_cap=None):
    """The clip in launches of `lengths` frames, frame numbers from `first`; rows with the clip's own frame indices."""
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker, rows_to_numpy
    kw, n_f = HANDLES[name]
    trk = DeviceTracker(capacity=cap, max_det=md, n_f=n_f, **kw)
    assert trk.batched
    if poison:
        _poison(trk)
    rows = torch.empty((rows_cap or len(per_frame) * cap) * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    pieces, f = [], 0
    for nb in lengths:
        if f >= len(per_frame):
            break
        nb = min(nb, len(per_frame) - f)
        det, cnt = _upload(torch, per_frame[f:f + nb], md)
        count.zero_()
        trk.run(det, cnt, first + f, rows, count)
        pieces.append(rows_to_numpy(rows, int(count.item())).copy())
        f += nb
    assert f == len(per_frame)
    torch.cuda.synchronize()
    assert trk.info()[2] == 0
    got = np.concatenate(pieces)
    got["frame"] -= first
    return got, trk


def _hooks():
    import ctypes
    from ysmr_amd import _lib
    L = _lib.lib()
    L.ysmr_debug_ring_poison.argtypes = [ctypes.c_void_p]
    L.ysmr_debug_ring_zero_line.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
    return L


def _poison(trk):
    assert _hooks().ysmr_debug_ring_poison(trk._handle) == 0


def _zero_line_words(trk):
    import ctypes
    n = ctypes.c_longlong(-1)
    assert _hooks().ysmr_debug_ring_zero_line(trk._handle, ctypes.byref(n)) == 0
    return n.value


def record(path):
    """Writes the recording (module docstring) with whatever library is loaded."""
    import torch
    out = {}
    for name in HANDLES:
        got, _ = _run(torch, name, refresh_clip(), [64] * N_FRAMES)
        out[name] = _recorded(got)
    np.savez_compressed(path, **out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HANDLES))
def test_same_bytes_as_before_the_grouped_refresh(oracle, name):
    """Cases 1 and 2: the rows of the recorded frames equal the recording byte for byte -- for launches of 64 / 7 / 1 frames and
    with frame 64 as a launch's first, last and an inner frame -- and every run is within compare_rows of the oracle."""
    import torch
    ref, live, ot = _oracle(oracle, name)
    want = golden(GOLDEN)[name]
    for cut, lengths in _cuts(N_FRAMES, REFRESH[0]).items():
        got, trk = _run(torch, name, refresh_clip(), lengths)
        compare_rows(got, ref)
        assert trk.info()[:2] == (int(live[-1]), ot.next_id)
        late = _recorded(got)
        assert late.dtype == want.dtype and len(late) == len(want), cut
        assert late.tobytes() == want.tobytes(), f"launches cut as '{cut}': rows differ from the recording"


@pytest.mark.gpu
@pytest.mark.parametrize("first", [5, 37, 4, 58])
@pytest.mark.parametrize("name", ["nf3", "short"])
def test_ring_wrap_in_every_group(oracle, name, first):
    """Case 3: the clip's frames numbered from `first`, so that frame 64 is the clip's frame 59, 27, 60 or 6 and the refresh
    meets the ring's head at 27, 27, 28 or 6 (numbered from 0 it is 0: the test above).  The entry of age a is at position
    (head - 1 - a) & 31, which wraps behind age 26 -- between two groups of three --, behind age 27 -- inside one -- and
    behind age 5, inside a group and inside the short handle's 13 ages.  The oracle knows no frame numbers: its rows are the
    clip's.  Byte for byte between the cuts."""
    import torch
    ref, live, ot = _oracle(oracle, name)
    per_frame = refresh_clip()
    runs = {}
    for cut, lengths in _cuts(N_FRAMES, REFRESH[0] - first).items():
        got, trk = _run(torch, name, per_frame, lengths, first=first)
        compare_rows(got, ref)
        runs[cut] = got.tobytes()
    assert len(set(runs.values())) == 1, {k: hash(v) for k, v in runs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nf3", "nf1", "short"])
def test_no_nan_leaves_the_ring(oracle, name):
    """Case 4: every ring position holds a NaN pattern before the first launch.  Entries at and beyond a track's history
    are requested -- by a young track, by the last group -- and never summed: no NaN in any row, the rows are the
    recording's, and the ring's line of zeros is still all zeros."""
    import torch
    ref, _, _ = _oracle(oracle, name)
    want = golden(GOLDEN)[name]
    for cut in ("64", "inner"):
        got, trk = _run(torch, name, refresh_clip(), _cuts(N_FRAMES, REFRESH[0])[cut], poison=True)
        assert not np.isnan(got["x"]).any() and not np.isnan(got["y"]).any(), f"launches cut as '{cut}': a NaN left the ring"
        compare_rows(got, ref)
        assert _recorded(got).tobytes() == want.tobytes()
        assert _zero_line_words(trk) == 0


@pytest.mark.gpu
def test_dead_lanes_and_helper_waves_at_the_refresh(oracle):
    """Case 5: 600 stationary tracks through a refresh frame -- nine full waves, a wave of 24 live and 40 dead lanes, two
    helper waves -- against the oracle, and the same bytes for one launch and for launches of 7 frames.  (40 frames, not
    130: the oracle's time goes with tracks x frames, and the waves' shape at the refresh is what the case is about.)"""
    import torch
    per_frame = stationary_clip()
    ref, live, ot = oracle_rows(oracle, per_frame, use_gsff=True, shadows=2, n_f=3, **KW)
    assert live.min() == live.max() == 600 and STATIONARY_FIRST < REFRESH[0] < STATIONARY_FIRST + STATIONARY_FRAMES
    runs = []
    for lengths in ([64], [7] * 6):
        got, trk = _run(torch, "nf3", per_frame, lengths, first=STATIONARY_FIRST, cap=768, md=640, rows_cap=len(ref) + 8)
        compare_rows(got, ref)
        assert trk.info()[:2] == (600, ot.next_id)
        runs.append(got.tobytes())
    assert runs[0] == runs[1]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
