"""The batch link's per-cell candidate lists (csrc/batch_link.h: k_bgrid builds, for every cell of a frame of <= 600
detections, the detections that can be nearest to a point of the cell; bl_search reads them) against the CPU oracle,
through ``ysmr_tracker_run``, on frames built to reach every branch: a single detection, a dense cluster beside lone
far tracks, lost tracks far outside the detections' bounding box (outside the grid: the 3 x 3 search), detections and
predictions on cell borders and grid edges with exact distance ties, lists at and over their cap of eight, 16, 32 and
48 cells per side (48: no lists), and empty frames between full ones."""
import numpy as np
import pytest

from conftest import compare_rows

pytestmark = pytest.mark.gpu


def _info(rng, n):
    return np.column_stack([rng.uniform(1, 9, n), rng.uniform(1, 9, n), rng.uniform(0, 90, n)])


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64).reshape(-1, 2)


def _ring(c, r, k):
    a = 2 * np.pi * np.arange(k) / k
    return np.column_stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)])


def candidate_clip(seed=5, ties=True):
    """[(xy (m,2), info (m,3)) per frame]; max_disappeared = 3 (four empty frames end every track).  ``ties=False``
    leaves out the two scenes of planted exact ties (C, D): with GSFF on, which of two equally distant tracks takes a
    detection hangs on the last bits of the gains (conftest.compare_rows), as in test_gpu_batch_link.py's tie tests."""
    rng = np.random.default_rng(seed)
    xy_frames = []
    empty = np.zeros((0, 2))
    rest = [empty] * 4

    # A: ~450 moving blobs (32 cells per side, as the bench), a dense cluster, three lone detections far away; dropout;
    # an empty frame in the middle
    pos = np.column_stack([rng.uniform(10, 1218, 450), rng.uniform(10, 912, 450)])
    vel = rng.normal(0, 1.0, pos.shape)
    cluster = rng.uniform(600, 630, (40, 2))
    lone = np.array([[5.0, 5.0], [1220.0, 10.0], [20.0, 915.0]])
    for f in range(10):
        pos = pos + vel
        keep = rng.random(len(pos)) > 0.05
        xy_frames.append(empty if f == 5 else np.vstack([pos[keep], cluster + 0.1 * f, lone]))
    xy_frames += rest

    # B: 300 blobs everywhere, then only those in a corner: the others' tracks are lost far outside the grid
    pos = np.column_stack([rng.uniform(0, 1200, 300), rng.uniform(0, 900, 300)])
    xy_frames.append(pos)
    corner = pos[(pos[:, 0] < 200) & (pos[:, 1] < 200)]
    for f in range(3):
        xy_frames.append(corner + 0.5 * (f + 1))
    xy_frames += rest

    # C: a lattice of pitch 32 on the cell borders (extent 960 = 30 cells of exactly 32 px), its two corners always
    # present; a frame without 60 of its points leaves their tracks with four neighbours at exactly the same distance
    lattice = np.stack(np.meshgrid(np.arange(31) * 32.0, np.arange(31) * 32.0), -1).reshape(-1, 2)
    pick = np.concatenate([[0, len(lattice) - 1], rng.choice(np.arange(1, len(lattice) - 1), 420, replace=False)])
    full = lattice[pick]
    gone = np.ones(len(full), bool)
    gone[2 + rng.choice(len(full) - 2, 60, replace=False)] = False
    if ties:
        xy_frames += [full, full[gone], full, full + np.array([16.0, 0.0]), full]
        xy_frames += rest

    # D: tracks at the centres of rings of 8 (a list at its cap) and of 12 (over it, with four exact ties each)
    centres = np.array([[100.0 + 300 * i, 100.0 + 250 * j] for i in range(4) for j in range(4)])
    if ties:
        xy_frames.append(centres)
        rings = [_ring(c, 12.0, 8 if k % 2 else 12) for k, c in enumerate(centres)]
        xy_frames += [np.vstack(rings), np.vstack(rings), centres]
        xy_frames += rest

    # E: one detection
    xy_frames += [np.array([[300.0, 200.0]]), np.array([[303.0, 201.0]]), empty, np.array([[306.0, 202.0]])]
    xy_frames += rest

    # F: 700 blobs (48 cells per side: the 3 x 3 search), G: 100 blobs (16 cells per side)
    for n in (700, 100):
        pos = np.column_stack([rng.uniform(10, 1218, n), rng.uniform(10, 912, n)])
        vel = rng.normal(0, 1.0, pos.shape)
        for f in range(3):
            pos = pos + vel
            xy_frames.append(pos[rng.random(n) > 0.03])
        xy_frames += rest
    return [(_f32(xy), np.asarray(_info(rng, len(xy)), np.float32).astype(np.float64)) for xy in xy_frames]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _run_frames(torch, trk, per_frame, batch, max_det, rows_cap):
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    rows = torch.empty(rows_cap * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for b0 in range(0, len(per_frame), batch):
        chunk = per_frame[b0:b0 + batch]
        det = torch.zeros(len(chunk), max_det, 5, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(len(chunk), dtype=torch.int32, device="cuda")
        for i, (d, info) in enumerate(chunk):
            if len(d):
                det[i, :len(d)] = torch.from_numpy(np.column_stack([d, info]).astype(np.float32)).cuda()
            cnt[i] = len(d)
        trk.run(det, cnt, b0, rows, count)
    torch.cuda.synchronize()
    assert trk.info()[2] == 0
    return rows_to_numpy(rows, int(count.item()))


def test_candidate_clip_reaches_every_grid_size():
    counts = [len(d) for d, _ in candidate_clip()]
    grid = [16 if m <= 128 else (32 if m <= 600 else 48) for m in counts if m]
    assert 0 in counts and 1 in counts and set(grid) == {16, 32, 48} and max(counts) <= 768


@pytest.mark.parametrize("use_gsff", [False, True])
def test_batch_link_with_candidate_lists_matches_oracle(torch_cuda, oracle, use_gsff):
    from link_clips import oracle_rows
    from ysmr_amd.tracker import DeviceTracker
    per_frame = candidate_clip(ties=not use_gsff)
    kw = dict(max_disappeared=3.0, fps=30.0, n_min=0, n_max=30, n_f=3, use_gsff=use_gsff)
    ref, live, ot = oracle_rows(oracle, per_frame, shadows=2 if use_gsff else 0, **kw)
    assert live.max() <= 768
    for batch in (256, 9):
        trk = DeviceTracker(capacity=768, max_det=1024, **kw)
        assert trk.batched
        got = _run_frames(torch_cuda, trk, per_frame, batch, 1024, len(ref) + 8)
        compare_rows(got, ref)
        assert trk.info()[:2] == (int(live[-1]), ot.next_id)
