"""The split candidate lists of the batch link (csrc/batch_link.h): k_bgrid gives a cell whose candidate list overflows the
lists of its four quadrants, in the overflow area behind the lists, and bl_search reads the list of the prediction's
quadrant.  Clips: tests/split_clips.py (crowded cells in general position, a ring of twelve at equal radii whose quadrants
still overflow, a frame with more crowded cells than overflow entries, tracks on the quadrants' midlines, within e of them
and crossing them from frame to frame); the model: tests/cell_list_model.py.

(a) the block k_bgrid leaves for a frame, read back with ysmr_debug_read_grid_block, against the model: header, cell
    starts, centres and columns (within a cell the device's order is that of its LDS atomics: compared as sets, and the
    model then lists the centres in the device's order), every cell's slot and every overflow entry;
(b) the rows of ysmr_tracker_run against the CPU oracle, GSFF on and off, whole clip in one launch and in batches of 3;
    once with max_det = 128, where the overflow area makes the block -- and the kernel's two buffers -- larger.
"""
import ctypes

import numpy as np
import pytest

import cell_list_model as M
from conftest import compare_rows
from split_clips import split_clip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module", params=[16, 32])
def clip(request):
    return request.param, split_clip(request.param)[0]


def _upload(torch, per_frame, max_det):
    det = torch.zeros(len(per_frame), max_det, 5, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(len(per_frame), dtype=torch.int32, device="cuda")
    for i, (d, info) in enumerate(per_frame):
        det[i, :len(d)] = torch.from_numpy(np.column_stack([d, info]).astype(np.float32)).cuda()
        cnt[i] = len(d)
    return det, cnt


def _read_block(trk, frame, dwords):
    from ysmr_amd import _lib
    L = _lib.lib()
    L.ysmr_debug_read_grid_block.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    L.ysmr_debug_read_grid_block.restype = ctypes.c_int
    out = np.zeros(dwords, np.uint32)
    assert L.ysmr_debug_read_grid_block(trk._handle, 0, frame, out.ctypes.data, out.nbytes) == 0, _lib.last_error()
    return out


def test_blocks_match_the_model(torch_cuda, clip):
    from ysmr_amd.tracker import DeviceTracker
    G, per_frame = clip
    max_det = 512
    trk = DeviceTracker(max_disappeared=30.0, fps=30.0, n_min=0, n_max=30, n_f=3, use_gsff=False, capacity=768, max_det=max_det)
    assert trk.batched
    det, cnt = _upload(torch_cuda, per_frame, max_det)
    trk.prepare(det, cnt, 0)
    seen = {"split": 0, "flagged": 0, "over": 0}
    for f, (xy, _) in enumerate(per_frame):
        m = len(xy)
        blk = _read_block(trk, f, M.grid_dwords(m))
        g, order = M.bin_frame(xy)
        assert g.G == G
        # header
        assert np.array_equal(blk[:4].view(np.float32), np.array([g.x0, g.y0, g.cell, g.inv], np.float32))
        assert blk[4:7].tolist() == [G, m, M.BL_LIST] and not blk[7:16].any()
        # cell starts
        at = 16
        start = blk[at:at + M.start_dwords(G)].view(np.uint16)
        assert np.array_equal(start[:G * G + 1], g.start)
        # centres and columns: the model's, cell by cell
        at += M.start_dwords(G)
        cen = blk[at:at + 2 * M.mp(m)].view(np.float32).reshape(-1, 2)
        at += 2 * M.mp(m)
        col = blk[at:at + M.mp(m) // 2].view(np.uint16)
        assert at + M.mp(m) // 2 == M.list_off(m)
        xy32 = np.asarray(xy, np.float32)
        assert np.array_equal(cen[:m], xy32[col[:m]]), "a centre is not its column's detection"
        assert np.all(cen[m:] == np.float32(1.0e30))
        for c in np.flatnonzero(np.diff(g.start)):
            assert sorted(col[g.start[c]:g.start[c + 1]].tolist()) == sorted(order[g.start[c]:g.start[c + 1]].tolist())
        # lists and overflow entries, from the centres in the device's order
        lists, over = M.frame_lists(g, cen[:m])
        got = blk[M.list_off(m):M.ovf_off(m)].view(np.uint16).reshape(G * G, M.BL_LIST)
        got_over = blk[M.ovf_off(m):M.ovf_off(m) + M.BL_OVF * 4 * M.BL_LIST // 2].view(np.uint16).reshape(M.BL_OVF, 4, M.BL_LIST)
        assert np.array_equal(got[:, 0], lists[:, 0]), "flags / markers / first candidates differ"
        plain = lists[:, 0] < M.SPLIT
        assert np.array_equal(got[plain], lists[plain])
        split = lists[:, 0] == M.SPLIT
        assert np.array_equal(got[split, 1], lists[split, 1]), "a split cell names another overflow entry"
        # (an overflow entry: a quadrant that still overflows is flagged in its first u16, the rest is not specified)
        fl = over[:, :, 0] == M.FLAG
        assert np.array_equal(got_over[:, :, 0], over[:, :, 0])
        assert np.array_equal(got_over[~fl], over[~fl])
        seen["split"] += int(split.sum())
        seen["flagged"] += int((lists[:, 0] == M.FLAG).sum())
        seen["over"] += int((lists[:, 0] >= M.SPLIT).sum() > M.BL_OVF)
    assert seen["split"] >= 8 and seen["flagged"] >= 8 and (G == 16 or seen["over"] >= 1)


def _run_frames(torch, trk, per_frame, batch, max_det, rows_cap):
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    rows = torch.empty(rows_cap * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for b0 in range(0, len(per_frame), batch):
        det, cnt = _upload(torch, per_frame[b0:b0 + batch], max_det)
        trk.run(det, cnt, b0, rows, count)
    torch.cuda.synchronize()
    assert trk.info()[2] == 0
    return rows_to_numpy(rows, int(count.item()))


@pytest.fixture(scope="module")
def oracle_ref(oracle):
    from link_clips import oracle_rows
    cache = {}

    def ref(G, per_frame, use_gsff):
        if (G, use_gsff) not in cache:
            kw = dict(max_disappeared=30.0, fps=30.0, n_min=0, n_max=30, n_f=3, use_gsff=use_gsff)
            cache[G, use_gsff] = oracle_rows(oracle, per_frame, shadows=2 if use_gsff else 0, **kw)
        return cache[G, use_gsff]
    return ref


@pytest.mark.parametrize("use_gsff", [False, True])
def test_rows_match_the_oracle(torch_cuda, oracle_ref, clip, use_gsff):
    from ysmr_amd.tracker import DeviceTracker
    G, per_frame = clip
    ref, live, ot = oracle_ref(G, per_frame, use_gsff)
    assert live.max() <= 300
    kw = dict(max_disappeared=30.0, fps=30.0, n_min=0, n_max=30, n_f=3, use_gsff=use_gsff)
    for batch in (len(per_frame), 3):
        trk = DeviceTracker(capacity=768, max_det=512, **kw)
        assert trk.batched
        got = _run_frames(torch_cuda, trk, per_frame, batch, 512, len(ref) + 8)
        compare_rows(got, ref)
        assert trk.info()[:2] == (int(live[-1]), ot.next_id)


def test_rows_match_the_oracle_where_the_overflow_area_sets_the_buffers(torch_cuda, oracle_ref):
    """max_det = 128: the largest block is that of 128 detections with lists, 1 536 dwords before the overflow area and
    1 792 with it -- k_batch's two buffers and everything behind them in LDS move."""
    from ysmr_amd.tracker import DeviceTracker
    per_frame = split_clip(16)[0]
    assert M.grid_dwords(128) == 1792 and max(len(d) for d, _ in per_frame) <= 128
    ref, live, ot = oracle_ref(16, per_frame, True)
    kw = dict(max_disappeared=30.0, fps=30.0, n_min=0, n_max=30, n_f=3, use_gsff=True)
    trk = DeviceTracker(capacity=768, max_det=128, **kw)
    assert trk.batched
    got = _run_frames(torch_cuda, trk, per_frame, len(per_frame), 128, len(ref) + 8)
    compare_rows(got, ref)
    assert trk.info()[:2] == (int(live[-1]), ot.next_id)
