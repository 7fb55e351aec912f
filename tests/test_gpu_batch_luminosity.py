"""GPU (run with -m gpu): the batch link of a 3-D handle -- ``ysmr_tracker_link_mode(t, 2)``, k_bgrid3 + k_batch3.

The reference is tests/luminosity_model.py::Linker (the model the per-frame 3-D tests use, itself pinned by
tests/golden/tracker_lum_*.npz).  Without a filter bank a row is raw coordinates: expected and actual tables are compared
byte for byte, and so are the batch and the per-frame path against each other.  There is no tolerance in this file.

Every test that uses a synthetic clip first asserts on the MODEL that the clip can show something: no decision of it hangs on
a distance gap below 1e-9 (``min_gap``), and the third coordinate decides at least one identity.
"""
import numpy as np
import pytest

import lum_batch_clips as LC
import luminosity_clips as C
import luminosity_model as M
from conftest import compare_rows, golden
from test_gpu_luminosity import _check_rows, _fixture_frames, _rows_from_table, _settings

pytestmark = pytest.mark.gpu

FIXTURES = ["tracker_lum_cross.npz", "tracker_lum_births.npz"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _tracker(max_disappeared, capacity, max_det, mode=2, fps=30.0):
    from ysmr_amd.tracker import DeviceTracker
    return DeviceTracker(max_disappeared=float(max_disappeared), fps=float(fps), use_gsff=False, capacity=capacity,
                         max_det=max_det, dimensions=3, link_mode=mode)


def _rows_buffer(torch, n_rows):
    from ysmr_amd import _lib
    return (torch.empty((n_rows + 8) * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
            torch.zeros(1, dtype=torch.int64, device="cuda"))


def _model_rows(per_frame, f0=0, f1=None):
    """The model's rows of frames [f0, f1) as a ysmr_row array."""
    from ysmr_amd import _lib
    flat = [r for rows in per_frame[f0:f1] for r in rows]
    out = np.zeros(len(flat), _lib.ROW_DTYPE)
    for k, r in enumerate(flat):
        out[k] = (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7])
    return out


def _fixture_arrays(g, max_det):
    """A fixture as ``run`` takes it; stale slots hold some detection's exact spot and a plausible luminosity."""
    frames = [(d, info.astype(np.float32)) for d, info in _fixture_frames(g)]
    assert np.array_equal(g["det"][:, :2].astype(np.float32).astype(np.float64), g["det"][:, :2]), "x, y must be float32 values"
    return LC.arrays(frames, max_det)


def _run_in_batches(torch, trk, det_d, third_d, counts_d, batch, rows, n, f_from=0):
    n_frames = det_d.shape[0]
    for f0 in range(f_from, n_frames, batch):
        f1 = min(f0 + batch, n_frames)
        trk.run(det_d[f0:f1], counts_d[f0:f1], f0, rows, n, third=third_d[f0:f1])
    torch.cuda.synchronize()


# ---- 1. the reference's fixtures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 64, None], ids=["1", "7", "64", "whole"])
@pytest.mark.parametrize("capacity,max_det", [(512, 512), (768, 2048)])
@pytest.mark.parametrize("name", FIXTURES)
def test_run3_through_the_batch_launch_matches_the_reference(torch_cuda, name, capacity, max_det, batch):
    torch = torch_cuda
    from ysmr_amd.tracker import rows_to_numpy
    g = golden(name)
    trk = _tracker(g["max_disappeared"], capacity, max_det, fps=float(g["fps"]))
    assert trk.batched and not trk.fused
    det, third, counts = _fixture_arrays(g, max_det)
    n_frames = len(counts)
    batch = batch or n_frames
    det_d, third_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(third).cuda(), torch.from_numpy(counts).cuda()
    total = int(g["off"][-1])
    rows, n = _rows_buffer(torch, total)
    _run_in_batches(torch, trk, det_d, third_d, counts_d, batch, rows, n)
    assert int(n.item()) == total
    _check_rows(rows_to_numpy(rows, total), g, 0, n_frames)
    ids, xyz, gone = trk.peek()
    sl = slice(g["off"][-2], g["off"][-1])
    assert list(ids) == list(g["ids"][sl]) and list(gone) == list(g["disappeared"][sl])
    assert xyz.shape == (len(ids), 3) and xyz.tobytes() == np.ascontiguousarray(g["xy"][sl]).tobytes()
    assert trk.info() == (len(ids), int(g["next_id"][-1]), 0)
    # reset keeps the dimension and the mode: the same frames give the same table again
    trk.reset()
    assert trk.batched
    n.zero_()
    k = min(batch, n_frames)
    trk.run(det_d[:k], counts_d[:k], 0, rows, n, third=third_d[:k])
    torch.cuda.synchronize()
    _check_rows(rows_to_numpy(rows, int(n.item())), g, 0, k)


# ---- 2. / 3. synthetic clips against the model -----------------------------------------------------------------------------
def _check_clip_against_the_model(torch, case, batch, capacity=768, max_det=2048):
    from ysmr_amd.tracker import rows_to_numpy
    frames = LC.clip3(*case)
    per_frame, (ids_m, pts_m, gone_m), next_id, min_gap, most = LC.model_table(*case)
    # the two preconditions, on the model
    assert min_gap >= 1e-9, f"the expected table hangs on a distance gap of {min_gap}"
    assert LC.identities_differ(per_frame, LC.model_table(*case, 2)[0]), "the third coordinate decides nothing on this clip"
    assert most <= capacity and max(len(p) for p, _ in frames) <= max_det
    trk = _tracker(LC.MAX_DISAPPEARED, capacity, max_det)
    assert trk.batched
    det, third, counts = LC.arrays(frames, max_det)
    det_d, third_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(third).cuda(), torch.from_numpy(counts).cuda()
    want = _model_rows(per_frame)
    rows, n = _rows_buffer(torch, len(want))
    _run_in_batches(torch, trk, det_d, third_d, counts_d, batch or len(frames), rows, n)
    assert int(n.item()) == len(want)
    got = rows_to_numpy(rows, len(want))
    for key in ("frame", "track_id", "disappeared"):      # (named first: a failure then says what differs)
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["x"].tobytes() == want["x"].tobytes() and got["y"].tobytes() == want["y"].tobytes()
    assert got.tobytes() == want.tobytes()
    ids, xyz, gone = trk.peek()
    assert list(ids) == ids_m and list(gone) == gone_m
    assert xyz.shape == (len(ids_m), 3) and xyz.tobytes() == np.ascontiguousarray(pts_m).tobytes()
    assert trk.info() == (len(ids_m), next_id, 0)
    return frames


CLIPS = [(48, 120, 1, 1), (48, 120, 1, 40), (40, 740, 2, 1), (40, 740, 2, 40)]


@pytest.mark.parametrize("batch", [16, None], ids=["16", "whole"])
@pytest.mark.parametrize("case", CLIPS, ids=lambda c: "-".join(str(v) for v in c))
def test_clip_through_the_batch_launch_matches_the_model(torch_cuda, case, batch):
    frames = _check_clip_against_the_model(torch_cuda, case, batch)
    if case[1] == 740:      # what the large clips are for: the 48-cell grid, the wave search without its float pre-pass, twelve waves
        assert min(len(p) for p, _ in frames) > 600
        assert LC.model_table(*case)[4] > 704


def test_thirds_beyond_4096_take_the_exact_search(torch_cuda):
    case = (48, 120, 1, 2000)
    frames = LC.clip3(*case)
    assert max(np.abs(p[:, 2]).max() for p, _ in frames) >= 4096.0 > min(np.abs(p[:, 2]).min() for p, _ in frames)
    _check_clip_against_the_model(torch_cuda, case, 16)


def _check_frames_against_the_linker(torch, frames, lk, per_frame, capacity, max_det):
    """The frames through ONE run call of a 3-D handle in link mode 2: rows, peek() and info() byte-equal to the linker
    that has seen them (lk) and to its rows (per_frame)."""
    from ysmr_amd.tracker import rows_to_numpy
    want = _model_rows(per_frame)
    trk = _tracker(LC.MAX_DISAPPEARED, capacity, max_det)
    assert trk.batched
    det, third, counts = LC.arrays(frames, max_det)
    rows, n = _rows_buffer(torch, len(want))
    trk.run(torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda(), 0, rows, n, third=torch.from_numpy(third).cuda())
    torch.cuda.synchronize()
    assert int(n.item()) == len(want)
    got = rows_to_numpy(rows, len(want))
    np.testing.assert_array_equal(got["track_id"], want["track_id"])
    assert got.tobytes() == want.tobytes()
    ids, xyz, gone = trk.peek()
    assert list(ids) == list(lk.objects) and list(gone) == [lk.disappeared[i] for i in ids]
    assert xyz.tobytes() == np.array([lk.objects[i] for i in ids]).tobytes()
    assert trk.info() == (len(ids), lk.next_id, 0)


def _bright_track_frames():
    """The other way into the exact search: a TRACK whose own third coordinate is at or above 4096 in frames whose
    detections all stay far below it.  A dozen stationary blobs, blob 0 at (100, 100) with luminosity 5000 in frame 0 only.
    In frame 2 two more blobs are missing and two detections appear near track 0: X = (103, 100, 1), the nearer in the
    plane, and Y = (100, 110, 40), the nearer in space (100 + 4960^2 < 9 + 4999^2).  Eleven detections meet twelve tracks: no
    births, track 0 claims Y and is an ordinary track from then on."""
    blobs = [(100.0, 100.0, 5000.0)] + [(220.0 + 97.0 * (k % 4) + 3.0 * k, 90.0 + 173.0 * (k // 4) + 7.0 * k, 0.5 + 0.25 * k)
                                         for k in range(11)]
    box = [(3.0 + k, 2.0, 10.0 * k) for k in range(12)]
    frame = lambda pts, bx: (np.array(pts), np.array(bx, np.float32))  # noqa: E731
    x, y = ((103.0, 100.0, 1.0), (1.0, 1.0, 0.0)), ((100.0, 110.0, 40.0), (2.0, 2.0, 0.0))
    keep = range(1, 10)
    planted = frame([blobs[k] for k in keep][:4] + [x[0]] + [blobs[k] for k in keep][4:] + [y[0]],
                    [box[k] for k in keep][:4] + [x[1]] + [box[k] for k in keep][4:] + [y[1]])
    after = frame(blobs[1:] + [y[0]], box[1:] + [y[1]])
    return [frame(blobs, box), frame(blobs[1:], box[1:]), planted, after, after], 4, 10      # (frames, column of X, of Y)


def test_a_track_whose_own_third_is_beyond_4096_takes_the_exact_search(torch_cuda):
    torch = torch_cuda
    frames, col_x, col_y = _bright_track_frames()
    assert all(np.abs(p[:, 2]).max() < 4096.0 for p, _ in frames[1:]), "frames 1.. must not carry the header flag"
    lk, lk2 = M.Linker(LC.MAX_DISAPPEARED), M.Linker(LC.MAX_DISAPPEARED)
    per_frame = []
    for f, (pts, box) in enumerate(frames):
        if f in (1, 2):
            assert lk.objects[0][2] >= 4096.0, "track 0 no longer holds the bright point"
        claims, _ = lk.update(pts, [tuple(float(v) for v in b) for b in box])
        claims2, _ = lk2.update(pts[:, :2], [tuple(float(v) for v in b) for b in box])
        if f == 2:      # the third coordinate decides: Y in space, X in the plane
            assert claims[0] == col_y and claims2[0] == col_x
        per_frame.append(lk.rows(f))
    assert lk.min_gap >= 1e-9, f"the expected table hangs on a distance gap of {lk.min_gap}"
    _check_frames_against_the_linker(torch, frames, lk, per_frame, 768, 2048)


def _clump_frames():
    """A run of the 3 x 3 block with more than five entries, and the nearest in space among its sixth and later.  A dozen
    stationary blobs, blob 0 at (100, 100) with luminosity 50.  In frame 2 blob 0 and six far blobs are missing and a clump
    of seven detections appears around track 0: six within 28 px in the plane but 29 to 31 away in luminosity, and
    Y = (108, 100, 51), 8 px away in the plane and the nearest in space (64 + 1 < 9 + 30^2).  The frame's bounding box is
    72 .. 520 in x and starts at 90 in y, so its 16 x 16 cells are 32 px wide with sides at 40 + 32 k and 58 + 32 k: track 0
    and the six lie in cell (1, 1), Y in cell (2, 1) -- behind all six in the row's run.  Twelve detections meet twelve
    tracks: no births, track 0 claims Y and is an ordinary track from then on."""
    blobs = [(100.0, 100.0, 50.0)] + [(220.0 + 97.0 * (k % 4) + 3.0 * k, 90.0 + 173.0 * (k // 4) + 7.0 * k, 0.5 + 0.25 * k)
                                       for k in range(11)]
    box = [(3.0 + k, 2.0, 10.0 * k) for k in range(12)]
    frame = lambda pts, bx: (np.array(pts), np.array(bx, np.float32))  # noqa: E731
    clump = [(97.0, 100.0, 80.0), (100.0, 104.0, 80.5), (96.0, 97.0, 79.5), (103.0, 106.0, 81.0), (94.0, 104.0, 79.0), (72.0, 96.0, 80.25)]
    y = (108.0, 100.0, 51.0)
    keep = [blobs[k] for k in range(1, 6)]
    pts = keep[:2] + clump[:3] + [y] + keep[2:] + clump[3:]
    bx = [box[k] for k in (1, 2)] + [(1.0, 1.0, 0.0)] * 3 + [(2.0, 2.0, 0.0)] + [box[k] for k in (3, 4, 5)] + [(1.0, 1.0, 0.0)] * 3
    after = frame(blobs[1:] + [y], box[1:] + [(2.0, 2.0, 0.0)])
    return [frame(blobs, box), frame(blobs, box), frame(pts, bx), after, after], 5      # (frames, column of Y)


def test_the_nearest_in_space_among_a_runs_sixth_and_later_candidates(torch_cuda):
    """bl_block_search's loop over a run's sixth and later candidates in three dimensions (`more`, q_extra): the one place
    where the search reads the f32 plane outside its fifteen unrolled loads."""
    torch = torch_cuda
    import cell_list_model as CL
    frames, col_y = _clump_frames()
    assert len(frames) <= 5 and all(np.abs(p[:, 2]).max() < 4096.0 for p, _ in frames), "the float stage must run"
    lk, lk2 = M.Linker(LC.MAX_DISAPPEARED), M.Linker(LC.MAX_DISAPPEARED)
    per_frame = []
    for f, (pts, box) in enumerate(frames):
        if f == 2:      # the preconditions, on the CPU: the frame's cells as k_bgrid3 makes them, track 0's 3 x 3 block
            assert len(pts) <= len(lk.objects), "a birth in the frame under test"
            xy32 = pts[:, :2].astype(np.float32)
            g, order = CL.bin_frame(xy32)
            cx, cy, _ = CL.lane_cell(g, lk.objects[0][0], lk.objects[0][1])
            assert 0 <= cx < g.G and 0 <= cy < g.G
            xl, xh = max(cx - 1, 0), min(cx + 1, g.G - 1)
            run0, run1 = int(g.start[cy * g.G + xl]), int(g.start[cy * g.G + xh + 1])
            assert run1 - run0 >= 7, "track 0's row of cells holds fewer than seven detections"
            nearest = int(M.cdist(lk.objects[0][None, :], pts)[0].argmin())
            assert nearest == col_y
            (pos,) = np.nonzero(order == nearest)[0]
            assert run0 <= pos < run1, "the nearest in space is not in the run of track 0's own row of cells"
            ccx = int(np.clip(np.floor((xy32[nearest, 0] - g.x0) * g.inv), 0, g.G - 1))
            first_of_its_cell = int(g.start[cy * g.G + ccx])
            # (order inside a cell is free on the device: every position its cell allows lies at or beyond the run's sixth)
            assert first_of_its_cell - run0 >= 5, "the nearest in space can come among the run's first five"
        claims, _ = lk.update(pts, [tuple(float(v) for v in b) for b in box])
        claims2, _ = lk2.update(pts[:, :2], [tuple(float(v) for v in b) for b in box])
        if f == 2:      # the third coordinate decides: Y in space, a member of the clump in the plane
            assert claims[0] == col_y and claims2[0] not in (col_y, -1)
        per_frame.append(lk.rows(f))
    assert lk.min_gap >= 1e-9, f"the expected table hangs on a distance gap of {lk.min_gap}"
    _check_frames_against_the_linker(torch, frames, lk, per_frame, 512, 512)


# ---- 4. an exact tie between two columns -----------------------------------------------------------------------------------
def _tie_frames(col_a, col_b):
    """A dozen stationary blobs; in frame 2 the blob of track 0 (at (100, 100), luminosity 1) and two far blobs are missing
    and two detections appear at exactly the same 3-D distance 5 from it: (103, 100, 5) and (100, 104, 4) -- 9 + 0 + 16 and
    0 + 16 + 9.  Eleven detections meet twelve tracks: no births, track 0 claims one of the two."""
    blobs = [(100.0, 100.0, 1.0)] + [(220.0 + 97.0 * (k % 4) + 3.0 * k, 90.0 + 173.0 * (k // 4) + 7.0 * k, 0.5 + 0.25 * k)
                                      for k in range(11)]
    box = [(3.0 + k, 2.0, 10.0 * k) for k in range(12)]
    full = (np.array(blobs), np.array(box, np.float32))
    keep = [k for k in range(12) if k not in (0, 10, 11)]
    pts = [blobs[k] for k in keep]
    bx = [box[k] for k in keep]
    extra = {col_a: ((103.0, 100.0, 5.0), (1.0, 1.0, 0.0)), col_b: ((100.0, 104.0, 4.0), (2.0, 2.0, 0.0))}
    for col in sorted(extra):
        pts.insert(col, extra[col][0])
        bx.insert(col, extra[col][1])
    tie = (np.array(pts), np.array(bx, np.float32))
    return [full, full, tie, full, full]


@pytest.mark.parametrize("col_a,col_b", [(3, 7), (7, 3)])
def test_two_columns_at_the_same_distance_lowest_column_wins(torch_cuda, col_a, col_b):
    torch = torch_cuda
    from ysmr_amd.tracker import rows_to_numpy
    frames = _tie_frames(col_a, col_b)
    lk = M.Linker(LC.MAX_DISAPPEARED)
    per_frame = []
    for f, (pts, box) in enumerate(frames):
        if lk.objects:      # no two ROWS tie for a column: the claim order is then the reference's whatever its argsort does
            D = M.cdist(np.array(list(lk.objects.values())), pts)
            arg, low = D.argmin(1), D.min(1)
            for c in np.unique(arg):
                assert len(set(low[arg == c])) == int((arg == c).sum()), f"two rows tie for column {c} in frame {f}"
            if f == 2:
                assert D[0, col_a] == D[0, col_b] == 5.0 == np.sort(D[0])[0], "the planted tie is not the row's minimum"
        claims, _ = lk.update(pts, [tuple(float(v) for v in b) for b in box])
        if f == 2:
            assert claims[0] == min(col_a, col_b), "argmin takes the lowest column"
        per_frame.append(lk.rows(f))
    want = _model_rows(per_frame)
    assert tuple(want[(want["frame"] == 2) & (want["track_id"] == 0)][["x", "y"]][0]) == \
        ((103.0, 100.0) if col_a < col_b else (100.0, 104.0))
    trk = _tracker(LC.MAX_DISAPPEARED, 768, 2048)
    assert trk.batched
    det, third, counts = LC.arrays(frames, 2048)
    rows, n = _rows_buffer(torch, len(want))
    trk.run(torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda(), 0, rows, n, third=torch.from_numpy(third).cuda())
    torch.cuda.synchronize()
    assert int(n.item()) == len(want)
    got = rows_to_numpy(rows, len(want))
    np.testing.assert_array_equal(got["track_id"], want["track_id"])
    assert got.tobytes() == want.tobytes()
    ids, xyz, _ = trk.peek()
    assert xyz.tobytes() == np.array([lk.objects[i] for i in ids]).tobytes()


# ---- 5. both paths, one table ----------------------------------------------------------------------------------------------
def test_batch_and_per_frame_paths_keep_one_table_through_switches(torch_cuda):
    torch = torch_cuda
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    case = (48, 120, 1, 40)
    frames = LC.clip3(*case)
    per_frame, _, _, min_gap, _ = LC.model_table(*case)
    assert min_gap >= 1e-9 and LC.identities_differ(per_frame, LC.model_table(*case, 2)[0])
    capacity, max_det = 768, 2048
    det, third, counts = LC.arrays(frames, max_det)
    det_d, third_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(third).cuda(), torch.from_numpy(counts).cuda()
    batch_only, frame_only, mixed = (_tracker(LC.MAX_DISAPPEARED, capacity, max_det, mode) for mode in (2, 1, 2))
    assert batch_only.batched and not frame_only.batched and mixed.batched
    total = sum(len(r) for r in per_frame)
    bufs = [_rows_buffer(torch, total) for _ in range(3)]
    one = torch.empty(capacity * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    n_one = torch.zeros(1, dtype=torch.int32, device="cuda")
    mixed_rows = []
    f0, mode, n_frames = 0, 2, len(frames)
    while f0 < n_frames:
        # a batch of seven through run: `mixed` in its current mode ...
        f1 = min(f0 + 7, n_frames)
        mixed.link_mode(mode)
        assert mixed.batched == (mode == 2)
        before = int(bufs[2][1].item())
        for trk, (rows, n) in zip((batch_only, frame_only, mixed), bufs):
            trk.run(det_d[f0:f1], counts_d[f0:f1], f0, rows, n, third=third_d[f0:f1])
        torch.cuda.synchronize()
        mixed_rows.append(rows_to_numpy(bufs[2][0], int(bufs[2][1].item()))[before:].copy())
        # ... then two single frames: `mixed` through update, the other two through run
        f2 = min(f1 + 2, n_frames)
        for f in range(f1, f2):
            m = int(counts[f])
            mixed.update(det_d[f, :max(m, 1)], m=m, frame=f, rows=one, n_rows=n_one, third=third_d[f])
            mixed_rows.append(rows_to_numpy(one, int(n_one.item())).copy())
            for trk, (rows, n) in zip((batch_only, frame_only), bufs[:2]):
                trk.run(det_d[f:f + 1], counts_d[f:f + 1], f, rows, n, third=third_d[f:f + 1])
        torch.cuda.synchronize()
        a = rows_to_numpy(bufs[0][0], int(bufs[0][1].item()))
        b = rows_to_numpy(bufs[1][0], int(bufs[1][1].item()))
        c = np.concatenate(mixed_rows)
        assert a.tobytes() == b.tobytes() == c.tobytes(), f"rows differ after frame {f2 - 1}"
        assert a.tobytes() == _model_rows(per_frame, 0, f2).tobytes()
        peeks = [trk.peek() for trk in (batch_only, frame_only, mixed)]
        for p in peeks[1:]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(peeks[0], p)), f"tables differ after frame {f2 - 1}"
        assert peeks[0][1].shape[1] == 3
        f0, mode = f2, 3 - mode
    assert len({trk.info() for trk in (batch_only, frame_only, mixed)}) == 1 and batch_only.info()[2] == 0


# ---- 6. prepare ------------------------------------------------------------------------------------------------------------
def test_prepare_on_a_side_stream_and_a_stale_block_is_not_used(torch_cuda):
    torch = torch_cuda
    from ysmr_amd.tracker import rows_to_numpy
    case = (48, 120, 1, 40)
    frames = LC.clip3(*case)
    per_frame, _, _, min_gap, _ = LC.model_table(*case)
    assert min_gap >= 1e-9 and LC.identities_differ(per_frame, LC.model_table(*case, 2)[0])
    max_det = 2048
    det, third, counts = LC.arrays(frames, max_det)
    det_d, third_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(third).cuda(), torch.from_numpy(counts).cuda()
    plain, prepared = _tracker(LC.MAX_DISAPPEARED, 768, max_det), _tracker(LC.MAX_DISAPPEARED, 768, max_det)
    total = sum(len(r) for r in per_frame)
    (rows_a, n_a), (rows_b, n_b) = _rows_buffer(torch, total), _rows_buffer(torch, total)
    side = torch.cuda.Stream()
    for k, f0 in enumerate(range(0, 32, 16)):
        sl = slice(f0, f0 + 16)
        plain.run(det_d[sl], counts_d[sl], f0, rows_a, n_a, third=third_d[sl])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            prepared.prepare(det_d[sl], counts_d[sl], k & 1, third=third_d[sl])
        torch.cuda.current_stream().wait_event(side.record_event())
        prepared.run(det_d[sl], counts_d[sl], f0, rows_b, n_b, third=third_d[sl])
    torch.cuda.synchronize()
    assert int(n_a.item()) == int(n_b.item()) == sum(len(r) for r in per_frame[:32])
    got = rows_to_numpy(rows_b, int(n_b.item()))
    assert got.tobytes() == rows_to_numpy(rows_a, int(n_a.item())).tobytes() == _model_rows(per_frame, 0, 32).tobytes()
    # a block prepared for buffers that an update then links from, and that are refilled, must not serve the next run
    buf_det, buf_third, buf_cnt = det_d[32:40].clone(), third_d[32:40].clone(), counts_d[32:40].clone()
    prepared.prepare(buf_det, buf_cnt, 0, third=buf_third)
    m = int(counts[32])
    one = torch.empty_like(rows_a[:768 * 40])
    n_one32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    prepared.update(buf_det[0, :m], m=m, frame=32, rows=one, n_rows=n_one32, third=buf_third[0])
    buf_det.copy_(det_d[33:41]); buf_third.copy_(third_d[33:41]); buf_cnt.copy_(counts_d[33:41])
    n_b.zero_()
    prepared.run(buf_det, buf_cnt, 33, rows_b, n_b, third=buf_third)
    torch.cuda.synchronize()
    assert rows_to_numpy(one, int(n_one32.item())).tobytes() == _model_rows(per_frame, 32, 33).tobytes()
    assert rows_to_numpy(rows_b, int(n_b.item())).tobytes() == _model_rows(per_frame, 33, 41).tobytes()


# ---- 7. handles the 3-D batch launch does not serve ---------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,max_det", [(1024, 1024), (512, 4096)])
@pytest.mark.parametrize("name", FIXTURES)
def test_ineligible_handles_keep_the_per_frame_link_in_mode_2(torch_cuda, name, capacity, max_det):
    torch = torch_cuda
    from ysmr_amd.tracker import rows_to_numpy
    g = golden(name)
    trk = _tracker(g["max_disappeared"], capacity, max_det, fps=float(g["fps"]))
    assert not trk.batched
    det, third, counts = _fixture_arrays(g, max_det)
    total = int(g["off"][-1])
    rows, n = _rows_buffer(torch, total)
    trk.run(torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda(), 0, rows, n, third=torch.from_numpy(third).cuda())
    torch.cuda.synchronize()
    assert int(n.item()) == total
    _check_rows(rows_to_numpy(rows, total), g, 0, len(counts))
    assert trk.info() == (int(g["off"][-1] - g["off"][-2]), int(g["next_id"][-1]), 0)


def test_an_eligible_3d_handle_is_not_batched_unless_asked(torch_cuda):
    trk = _tracker(5.0, 768, 2048, mode=0)
    assert trk.fused and not trk.batched
    trk.link_mode(2)
    assert trk.batched and not trk.fused
    trk.link_mode(1)
    assert trk.fused and not trk.batched
    trk.link_mode(0)
    assert trk.fused and not trk.batched
    from ysmr_amd.tracker import DeviceTracker
    flat = DeviceTracker(fps=30.0, use_gsff=False, capacity=768, max_det=2048, link_mode=2)      # on a 2-D handle mode 2 is mode 0
    assert flat.batched


def test_the_2d_prepare_stays_a_no_op_on_a_3d_handle(torch_cuda):
    """What a caller written before link mode 2 does -- prepare without a third coordinate ahead of run3 -- still succeeds
    in every mode, and the run that follows bins the batch itself."""
    torch = torch_cuda
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    g = golden(FIXTURES[0])
    det, third, counts = _fixture_arrays(g, 2048)
    det_d, third_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(third).cuda(), torch.from_numpy(counts).cuda()
    total = int(g["off"][-1])
    for mode in (0, 1, 2):
        trk = _tracker(g["max_disappeared"], 768, 2048, mode, fps=float(g["fps"]))
        rc = _lib.lib().ysmr_tracker_prepare(trk._handle, _lib.stream_ptr("cuda:0"), det_d.data_ptr(), counts_d.data_ptr(), len(counts), 0)
        assert rc == _lib.YSMR_OK
        assert trk.prepare(det_d, counts_d, 1) is None
        rows, n = _rows_buffer(torch, total)
        trk.run(det_d, counts_d, 0, rows, n, third=third_d)
        torch.cuda.synchronize()
        assert int(n.item()) == total
        _check_rows(rows_to_numpy(rows, total), g, 0, len(counts))


# ---- 8. the pipeline -------------------------------------------------------------------------------------------------------
def test_track_bacteria_with_luminosity_links_through_the_batch_launch(tmp_path, oracle):
    from ysmr_amd import track_eval
    frames = C.crossing_clip()
    ref, lk = C.expected_rows(oracle, frames, 30.0, dims=3, adt=2.0)
    assert lk.min_gap >= 1e-9, f"the expected table hangs on a distance gap of {lk.min_gap}"
    assert C.tracks_differ(ref, C.expected_rows(oracle, frames, 30.0, dims=2, adt=2.0)[0]), "the third coordinate decides nothing"
    path = tmp_path / "pairs.npy"
    np.save(path, frames)
    res = track_eval.track_bacteria(str(path), settings=_settings(**{"adaptive double threshold": 2.0}), result_folder=str(tmp_path), batch=16, max_det=256, capacity=256)
    assert res is not None
    assert track_eval.LAST_PIPELINE_FACTS["batched"] is True
    compare_rows(_rows_from_table(res[0], ref), [r[:7] for r in ref])
