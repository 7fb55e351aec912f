"""The batch link's claims (csrc/batch_link.h, k_batch: "claims") where its short key cannot decide.

A frame settles a detection column with ONE atomic minimum on (squared distance s without its ten lowest bits, table
row); two proposals whose s agree in the 54 bits kept, or differ by one step there, send the frame through the exact
rule (full s, rounded roots, id).  Every crafted pair below is asserted IN NUMPY, before the GPU sees it, to have the
bit pattern its case is about, and the expected winner comes from the reference's rule written out here
(tracker.py:151-163: ascending row minimum ``sqrt(s)``, then table row = ascending id) -- not from any kernel.

No GSFF in the crafted clips: a track's position is then its last measurement, a float32 that converts exactly, so s is
the float64 ``dx * dx + dy * dy`` of exact differences and numpy forms the same number as the kernel.

Every clip runs through k_batch with batches of 64 / 7 / 1 frames, through the per-frame link of the same kind of
handle (``link_mode(1)``) and through the host-side ``CentroidTracker``; ids, counters, row order and coordinates must
be EQUAL.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAMPS_LIB = os.path.join(ROOT, "scripts", "var_stamps.so")     # scripts/build_stamps.sh (not part of build())
BL_WAVES, BL_COUNTS, EXACT_COLUMN = 12, 9, 8                    # g_bcounts of the stamps build (batch_link.h)
MAX_GONE = 2.0
D = (1100.0, 8.0)                                               # the contested detection of most cases


# ---- numpy side: the numbers as the kernel forms them ----------------------------------------------------------------
def _f32(v):
    """v as float64, asserted to be a float32 value."""
    a = np.asarray(v, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f"{v} is not a float32 value"
    return a


def _s(p, d):
    """bl_dist2: s = dx * dx, then s + dy * dy, in float64 (no fused multiply-add), of exact differences."""
    dx = np.float64(p[0]) - np.float64(d[0])
    dy = np.float64(p[1]) - np.float64(d[1])
    s = dx * dx
    return s + dy * dy


def _bits(s):
    return int(np.float64(s).view(np.uint64))


def _field(s):
    """The 54 bits of s that the short key keeps."""
    return _bits(s) >> 10


def _reference_winner(contenders, d):
    """contenders: [(id, position)] all proposing detection d.  tracker.py:151-163: rows sorted by their minimum
    DISTANCE (the rounded root), a stable sort of rows in ascending id -> the smallest (sqrt(s), id)."""
    return min(contenders, key=lambda c: (float(np.sqrt(_s(c[1], d))), c[0]))[0]


# ---- clips ------------------------------------------------------------------------------------------------------------
BYSTANDERS = np.array([(2400.0 + 60.0 * i, 1000.0 + 60.0 * j) for j in range(5) for i in range(5)])
FAR_AWAY = (3400.0, 3000.0)


def _frame(points, seed):
    xy = _f32(np.array(points, np.float64).reshape(-1, 2))
    rng = np.random.default_rng(seed)
    info = np.column_stack([rng.uniform(1, 9, len(xy)), rng.uniform(1, 9, len(xy)), rng.uniform(0, 90, len(xy))])
    return xy, info.astype(np.float32).astype(np.float64)


def _contest_clip(lo, hi, d, swap, extra=None):
    """Tracks ``lo`` (the lower id) and ``hi`` -- and ``extra``, a third with the highest id -- lose their own
    detections and all find ``d`` nearest, for two frames; 25 stationary bystanders keep theirs throughout (nearer to
    themselves than to anything else, farther than 1300 px from the contenders and from d).
    swap=False: lo and hi are born in frame 0, in this order: ids 0, 1, seats (lanes of k_batch) 0, 1.
    swap=True:  a track born before ``lo`` sits in seat 0 and dies (3 frames unseen, max_disappeared = 2); ``hi`` is born
                afterwards and takes the lowest free seat, 0: the HIGHER id then sits in the LOWER seat, and its atomic
                comes first within the wave.
    Returns (frames, contest frame, {name: id})."""
    by = [tuple(p) for p in BYSTANDERS]
    late = [hi] + ([extra] if extra is not None else [])
    if not swap:
        frames = [[lo] + late + by]
        ids = {"lo": 0, "hi": 1, "extra": 2}
    else:
        frames = [[FAR_AWAY, lo] + by] + [[lo] + by] * 3 + [[lo] + by + late]
        ids = {"lo": 1, "hi": 2 + len(by), "extra": 3 + len(by)}
    contest = len(frames)
    frames += [[d] + by] * 2
    return [_frame(p, 100 + k) for k, p in enumerate(frames)], contest, ids


def _blob_clip(n_blobs=500, n_frames=64, seed=5):
    """An ordinary clip: ~500 moving blobs, 4 % dropout, a few births."""
    rng = np.random.default_rng(seed)
    pos = np.column_stack([rng.uniform(20, 1200, n_blobs), rng.uniform(20, 900, n_blobs)])
    vel = rng.normal(0, 1.0, (n_blobs, 2))
    frames = []
    for f in range(n_frames):
        pos = pos + vel + rng.normal(0, 0.2, pos.shape)
        xy = pos[rng.random(n_blobs) > 0.04]
        if f % 11 == 5:
            xy = np.vstack([xy, rng.uniform(1300, 1600, (4, 2))])
        xy = xy.astype(np.float32).astype(np.float64)
        info = np.column_stack([rng.uniform(1, 9, len(xy)), rng.uniform(1, 9, len(xy)), rng.uniform(0, 90, len(xy))])
        frames.append((xy, info.astype(np.float32).astype(np.float64)))
    return frames


# ---- GPU side ---------------------------------------------------------------------------------------------------------
def _run(trk, per_frame, batch, max_det, after_launch=None):
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    cap = sum(len(d) for d, _ in per_frame) * 2 + 64
    rows = torch.empty(cap * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for b0 in range(0, len(per_frame), batch):
        chunk = per_frame[b0:b0 + batch]
        det = torch.zeros(len(chunk), max_det, 5, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(len(chunk), dtype=torch.int32, device="cuda")
        for i, (d, info) in enumerate(chunk):
            det[i, :len(d)] = torch.from_numpy(np.column_stack([d, info]).astype(np.float32)).cuda()
            cnt[i] = len(d)
        trk.run(det, cnt, b0, rows, count)
        if after_launch is not None:
            torch.cuda.synchronize()
            after_launch()
    torch.cuda.synchronize()
    assert trk.info()[2] == 0
    return rows_to_numpy(rows, int(count.item())).copy()


INT_KEYS = ("frame", "track_id", "disappeared", "w", "h", "angle")


def _assert_rows_equal(a, b, what, xy_tol=None):
    assert len(a) == len(b), what
    for key in INT_KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")
    for key in ("x", "y"):
        if xy_tol is None:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")
        else:
            np.testing.assert_allclose(a[key], b[key], rtol=xy_tol, atol=xy_tol, err_msg=f"{what}: {key}")


def _all_ways(per_frame, capacity=128, max_det=64):
    """The clip (no GSFF) through k_batch in batches of 64 / 7 / 1, the per-frame link and the host tracker: equal rows."""
    from ysmr_amd.tracker import CentroidTracker, DeviceTracker
    kw = dict(max_disappeared=MAX_GONE, fps=30.0, use_gsff=False)
    rows = None
    for batch in (64, 7, 1):
        trk = DeviceTracker(capacity=capacity, max_det=max_det, **kw)
        assert trk.batched
        got = _run(trk, per_frame, batch, max_det)
        if rows is None:
            rows = got
        _assert_rows_equal(got, rows, f"k_batch, batches of {batch} against 64")
    one = DeviceTracker(capacity=capacity, max_det=max_det, **kw)
    one.link_mode(1)
    assert not one.batched
    _assert_rows_equal(_run(one, per_frame, 16, max_det), rows, "per-frame link against k_batch")
    host = CentroidTracker(capacity=capacity, max_det=max_det, **kw)
    at = 0
    for f, (d, info) in enumerate(per_frame):
        objects, _ = host.update([((float(x), float(y)), [float(v) for v in i3]) for (x, y), i3 in zip(d, info)])
        gone = host.disappeared
        part = rows[at:at + len(objects)]
        at += len(objects)
        assert np.all(part["frame"] == f), f"host tracker: rows of frame {f}"
        assert list(objects) == part["track_id"].tolist(), f"host tracker: ids and row order in frame {f}"
        np.testing.assert_array_equal(np.array([objects[t] for t in objects]).reshape(-1, 2),
                                      np.column_stack([part["x"], part["y"]]), err_msg=f"host tracker: frame {f}")
        assert [gone[t] for t in objects] == part["disappeared"].tolist(), f"host tracker: counters in frame {f}"
    assert at == len(rows)
    return rows


def _check_contest(lo, hi, d, swap, extra=None):
    """Runs the clip every way and holds the contest frame against the reference's rule."""
    lo, hi, d = tuple(_f32(lo)), tuple(_f32(hi)), tuple(_f32(d))
    extra = None if extra is None else tuple(_f32(extra))
    per_frame, contest, ids = _contest_clip(lo, hi, d, swap, extra)
    where = {ids["lo"]: lo, ids["hi"]: hi}
    if extra is not None:
        where[ids["extra"]] = extra
    winner = _reference_winner(sorted(where.items()), d)
    rows = _all_ways(per_frame)
    fr = rows[rows["frame"] == contest]
    assert fr["track_id"].tolist() == sorted(fr["track_id"].tolist())            # table order = ascending id
    for tid, p in where.items():
        r = fr[fr["track_id"] == tid]
        assert len(r) == 1
        if tid == winner:
            assert (r["x"][0], r["y"][0], r["disappeared"][0]) == (d[0], d[1], 0), f"track {tid} should have won"
        else:
            assert (r["x"][0], r["y"][0], r["disappeared"][0]) == (p[0], p[1], 1), f"track {tid} should have lost"
    return winner, ids


@pytest.mark.parametrize("swap", [False, True])
def test_equal_distances_go_to_the_lower_id(swap):
    """Case 1: two tracks at exactly the same s from one detection; the higher id in the higher seat and in the lower."""
    lo, hi = (D[0] - 3.0, D[1] + 4.0), (D[0] + 4.0, D[1] - 3.0)
    assert _s(lo, D) == _s(hi, D) == 25.0
    winner, ids = _check_contest(lo, hi, D, swap)
    assert winner == ids["lo"]


@pytest.mark.parametrize("swap", [False, True])
def test_same_high_bits_smaller_distance_wins_against_the_lower_id(swap):
    """Case 2: dx = 1024, dy = 0 against dx = 1024, dy = 2^-12 -- the same 54 high bits of s, different s, different
    roots.  The larger s goes to the LOWER id: the short key alone would give it the column."""
    lo, hi = (D[0] - 1024.0, D[1] + 2.0 ** -12), (D[0] - 1024.0, D[1])
    s_lo, s_hi = _s(lo, D), _s(hi, D)
    assert s_hi == 2.0 ** 20 and s_lo > s_hi and _field(s_lo) == _field(s_hi)
    assert np.sqrt(s_lo) != np.sqrt(s_hi)
    winner, ids = _check_contest(lo, hi, D, swap)
    assert winner == ids["hi"]


def _straddling_pair():
    """Offsets (dx, dy_a), (dx, dy_b) from a detection at y = 0.5, float32 all, whose s are a few ulps apart on the two
    sides of a truncation boundary: dx = 1024, dy = j 2^-24 gives s = 2^20 + j^2 2^-48, the boundary at j = 2^13."""
    found = None
    for ja in range(8192 - 64, 8192):
        for jb in range(8192, 8192 + 64):
            sa, sb = _s((1024.0, ja * 2.0 ** -24), (0.0, 0.0)), _s((1024.0, jb * 2.0 ** -24), (0.0, 0.0))
            if _field(sb) == _field(sa) + 1 and 0 < _bits(sb) - _bits(sa) <= 4:
                if found is None or _bits(sb) - _bits(sa) < found[0]:
                    found = (_bits(sb) - _bits(sa), ja * 2.0 ** -24, jb * 2.0 ** -24)
    assert found is not None
    return found[1], found[2]


@pytest.mark.parametrize("swap", [False, True])
def test_pair_across_a_truncation_boundary(swap):
    """Case 3: s a few ulps apart whose 54-bit fields differ by one step; the slightly larger s goes to the lower id.
    Whether the roots round to the same double is left to numpy: the expected winner follows the reference's rule."""
    dy_small, dy_large = _straddling_pair()
    d = (1100.0, 0.5)
    lo, hi = (d[0] - 1024.0, d[1] + dy_large), (d[0] - 1024.0, d[1] - dy_small)
    s_lo, s_hi = _s(lo, d), _s(hi, d)
    assert s_lo > s_hi and _bits(s_lo) - _bits(s_hi) <= 4 and _field(s_lo) == _field(s_hi) + 1
    winner, ids = _check_contest(lo, hi, d, swap)
    assert winner == (ids["lo"] if np.sqrt(s_lo) == np.sqrt(s_hi) else ids["hi"])


@pytest.mark.parametrize("swap", [False, True])
def test_different_distances_with_equal_rounded_roots_go_to_the_lower_id(swap):
    """Case 4: float32 coordinates inside a 1228 x 922 frame admit such a pair: dx = 1024, dy = 0 and dy = 2^-16 give
    s = 2^20 and 2^20 + 2^-32, one ulp apart, and sqrt(2^20 + 2^-32) = 1024 (1 + 2^-53 - ...) rounds to 1024.  The larger
    s goes to the lower id, which wins: the reference compares the rounded roots."""
    lo, hi = (D[0] - 1024.0, D[1] + 2.0 ** -16), (D[0] - 1024.0, D[1])
    for p in (lo, hi, D):
        assert 0.0 <= p[0] < 1228.0 and 0.0 <= p[1] < 922.0
    s_lo, s_hi = _s(lo, D), _s(hi, D)
    assert _bits(s_lo) == _bits(s_hi) + 1 and np.sqrt(s_lo) == np.sqrt(s_hi) == 1024.0
    winner, ids = _check_contest(lo, hi, D, swap)
    assert winner == ids["lo"]


@pytest.mark.parametrize("swap", [False, True])
def test_third_contender_far_below_a_near_equal_pair_wins(swap):
    """Case 5: two near-equal proposals (one ulp apart) and a third with a much smaller s and the highest id.  Whether the
    pair raises the frame's flag depends on the order of the atomics; the far one wins either way."""
    lo, hi, extra = (D[0] - 1024.0, D[1] + 2.0 ** -16), (D[0] - 1024.0, D[1]), (D[0] - 10.0, D[1])
    s_lo, s_hi, s_x = _s(lo, D), _s(hi, D), _s(extra, D)
    assert _field(s_lo) == _field(s_hi) and s_x == 100.0 and _field(s_x) + 2 < _field(s_hi)
    winner, ids = _check_contest(lo, hi, D, swap, extra=extra)
    assert winner == ids["extra"]


def _exact_path_frames(per_frame, batch, capacity, max_det, use_gsff):
    """Frames that took the exact claim path, counted by the stamps build (this process must have loaded it)."""
    import ctypes
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker
    L = _lib.lib()
    buf = (ctypes.c_ulonglong * (BL_WAVES * BL_COUNTS))()
    total = [0]

    def after_launch():
        assert L.ysmr_debug_read_bcounts(buf) == 0
        total[0] += int(np.array(buf[:], dtype=np.int64).reshape(BL_WAVES, BL_COUNTS)[:, EXACT_COLUMN].sum())

    trk = DeviceTracker(max_disappeared=MAX_GONE if not use_gsff else 8.0, fps=30.0, use_gsff=use_gsff, capacity=capacity,
                        max_det=max_det)
    assert trk.batched
    _run(trk, per_frame, batch, max_det, after_launch)
    return total[0]


def _stamps_child():
    """Runs in a process of its own with the stamps build loaded (YSMR_HIP_LIB): prints the counts as JSON."""
    tie, _, _ = _contest_clip((D[0] - 3.0, D[1] + 4.0), (D[0] + 4.0, D[1] - 3.0), D, False)
    print(json.dumps({"ordinary": _exact_path_frames(_blob_clip(), 64, 768, 1024, True),
                      "tie": _exact_path_frames(tie, 64, 128, 64, False)}))


def test_ordinary_clip_is_batch_invariant_and_never_takes_the_exact_path():
    """Cases 6 and 7 on a 500-blob clip with the filter bank on: batches of 64 / 7 / 1 give identical rows, the per-frame
    link the same ids, counters and row order (positions to 1e-9: its filter bank sums in another order).  Where the
    stamps build is present (scripts/build_stamps.sh) its counter says that no frame of the clip took the exact claim
    path -- and that the contest frame of an exact tie did, so the counter is known to count."""
    from ysmr_amd.tracker import DeviceTracker
    per_frame = _blob_clip()
    kw = dict(max_disappeared=8.0, fps=30.0, n_min=0, n_max=30, n_f=3, capacity=768, max_det=1024)
    rows = None
    for batch in (64, 7, 1):
        trk = DeviceTracker(**kw)
        assert trk.batched
        got = _run(trk, per_frame, batch, 1024)
        if rows is None:
            rows = got
        _assert_rows_equal(got, rows, f"k_batch, batches of {batch} against 64")
    assert 400 < np.sum(rows["frame"] == len(per_frame) - 1) <= 768
    one = DeviceTracker(**kw)
    one.link_mode(1)
    assert not one.batched
    _assert_rows_equal(_run(one, per_frame, 16, 1024), rows, "per-frame link against k_batch", xy_tol=1e-9)
    if os.path.exists(STAMPS_LIB):
        env = dict(os.environ, YSMR_HIP_LIB=STAMPS_LIB)
        code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.dirname(os.path.abspath(__file__))!r}]; import test_gpu_batch_claims as t; t._stamps_child()"
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        counts = json.loads(out.stdout.strip().splitlines()[-1])
        print("frames on the exact claim path:", counts)
        assert counts["ordinary"] == 0
        assert counts["tie"] >= 1
