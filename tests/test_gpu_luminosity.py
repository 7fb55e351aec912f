"""GPU (run with -m gpu): luminosity as a third tracking coordinate -- k_luminosity against the NumPy model
(tests/luminosity_model.py), the 3-D link against fixtures written by the reference's own tracker.py
(tests/golden/tracker_lum_*.npz), and 'include luminosity in tracking calculation' end to end.

Everything the kernel produces is compared as integers (corners, sums, counts) or as equal doubles; the link's ids,
claims, counters and positions are exact (no filter is involved in three dimensions).
"""
import ctypes
import logging
import os

import numpy as np
import pytest

import luminosity_clips as C
import luminosity_model as M
from conftest import compare_rows, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- 7. the kernel against the model ---------------------------------------------------------------------------------------
def _scene(height, width, seed, colour):
    """Blobs of every kind the kernel has cases for: rods at all angles, bars lying on all four borders and in the
    corners, single pixels, and one island taller than a wave has lanes (and than a group of 16 has, several times)."""
    from ysmr_amd.synth import SyntheticVideo
    rng = np.random.default_rng(seed)
    f = SyntheticVideo(height, width, 30, seed=seed, dropout=0.0, speckle=0.2).frames(1)[0].astype(np.int32)
    f[0:2, 10:19] = 200                     # top border
    f[height - 1, 30:37] = 210              # bottom border, one row
    f[20:29, 0:2] = 190                     # left border
    f[40:44, width - 1] = 205               # right border, one column
    f[0, 0] = f[height - 1, width - 1] = f[0, width - 1] = 220      # corners
    for (y, x) in ((50, 8), (8, 60), (90, 20), (70, 6)):            # faint single pixels: the blur leaves one pixel above the level
        f[y, x] = 76
    yy, xx = np.mgrid[0:height, 0:width]
    u = (xx - width * 0.62) * 0.8 + (yy - height * 0.5) * 0.6
    v = -(xx - width * 0.62) * 0.6 + (yy - height * 0.5) * 0.8
    island = (u / 14.0) ** 2 + (v / 45.0) ** 2 <= 1.0         # a tilted ellipse ~90 rows tall
    f[island] = 150 + (rng.integers(0, 60, f.shape))[island]
    f = np.clip(f, 0, 255).astype(np.uint8)
    if not colour:
        return f
    tint = rng.uniform(0.55, 1.0, 3)
    return np.clip(f[..., None] * tint + rng.integers(0, 9, f.shape + (3,)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("height,width,colour,flavour", [(112, 160, False, 0), (112, 160, False, 1), (101, 131, False, 0),
                                                         (112, 160, True, 0), (101, 131, True, 3)])
def test_kernel_equals_the_model_in_integers(torch_cuda, oracle, height, width, colour, flavour):
    """flavour: bit 0 the pre-4.5.1 angle convention (in the detections), bit 1 the 3.x gray coefficients (BGR frames).
    131 columns: rows start at every byte offset of a dword."""
    torch = torch_cuda
    from ysmr_amd import _lib
    frames = np.stack([_scene(height, width, 40 + k, colour) for k in range(3)])
    dets = [oracle.detect_frame(fr, cv_flavour=flavour).det for fr in frames]
    counts = np.array([len(d) for d in dets], np.int32)
    assert counts.min() > 20
    max_det = int(counts.max()) + 5
    det = np.zeros((3, max_det, 5), np.float32)
    for k, d in enumerate(dets):
        det[k, :len(d)] = d
    sizes = det[..., 2] * det[..., 3]
    assert sizes.max() > 64 * 20 and (det[..., 2:4].max(axis=-1)[sizes > 0] > 64).any(), "no island taller than a wave"
    assert any(((d[:, 2] == 0) & (d[:, 3] == 0)).any() for d in dets), "no single-pixel blob"
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    frames_d, det_d, counts_d = dev(frames), dev(det), dev(counts)
    lum = torch.full((3, max_det), -1.0, dtype=torch.float64, device="cuda")
    total = torch.full((3, max_det), -1, dtype=torch.int32, device="cuda")
    count = torch.full((3, max_det), -1, dtype=torch.int32, device="cuda")
    corners = torch.full((3, max_det, 4, 2), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().ysmr_luminosity_batch(_lib.stream_ptr("cuda:0"), frames_d.data_ptr(), 3, height, width, 3 if colour else 1,
                                          det_d.data_ptr(), counts_d.data_ptr(), max_det, flavour, lum.data_ptr(),
                                          total.data_ptr(), count.data_ptr(), corners.data_ptr())
    _lib.check(rc, "ysmr_luminosity_batch")
    torch.cuda.synchronize()
    lum, total, count, corners = lum.cpu().numpy(), total.cpu().numpy(), count.cpu().numpy(), corners.cpu().numpy()
    touched = set()
    for k in range(3):
        n = counts[k]
        gray = frames[k] if not colour else M.bgr2gray(frames[k], gray_3x=bool(flavour & 2))
        mc, ms, mn, ml = M.luminosity_frame(gray, det[k, :n])
        np.testing.assert_array_equal(corners[k, :n], mc, err_msg=f"corners, frame {k}")
        np.testing.assert_array_equal(count[k, :n].view(np.uint32), mn, err_msg=f"count, frame {k}")
        np.testing.assert_array_equal(total[k, :n].view(np.uint32), ms, err_msg=f"sum, frame {k}")
        assert lum[k, :n].tobytes() == ml.tobytes(), f"lum, frame {k}"
        assert (lum[k, n:] == -1.0).all() and (count[k, n:] == -1).all() and (corners[k, n:] == -7).all(), "slots past the count"
        xs, ys = mc[..., 0], mc[..., 1]
        touched |= {s for s, hit in (("left", (xs.min(1) <= 0)), ("right", (xs.max(1) >= width - 1)),
                                     ("top", (ys.min(1) <= 0)), ("bottom", (ys.max(1) >= height - 1))) if hit.any()}
    assert touched == {"left", "right", "top", "bottom"}


def test_detector_luminosity_of_its_own_detections(torch_cuda):
    """``Detector(luminosity=True)``: ``detect`` leaves ``DetectResult.lum``; the model applied to the DEVICE's detections
    (whose angles may sit an ulp from the oracle's) gives the same integers and the same doubles."""
    torch = torch_cuda
    from ysmr_amd.detect import Detector
    from ysmr_amd.synth import SyntheticVideo
    frames = SyntheticVideo(200, 260, 40, seed=3).frames(8)
    det = Detector(8, 200, 260, max_det=256, luminosity=True)
    plain = Detector(8, 200, 260, max_det=256)
    dev = torch.from_numpy(frames).cuda()
    res = det.detect(dev)
    assert plain.detect(dev).lum is None and res.lum is not None and res.lum.shape == (8, 256)
    sums = torch.zeros(8, 256, dtype=torch.int32, device="cuda")
    counts = torch.zeros(8, 256, dtype=torch.int32, device="cuda")
    corners = torch.zeros(8, 256, 4, 2, dtype=torch.int32, device="cuda")
    again = det.luminosity(dev, sums=sums, counts=counts, corners=corners)
    torch.cuda.synchronize()
    n, d, lum = res.det_count.cpu().numpy(), res.det.cpu().numpy(), res.lum.cpu().numpy()
    assert np.array_equal(again.cpu().numpy(), lum)
    for k in range(8):
        mc, ms, mn, ml = M.luminosity_frame(frames[k], d[k, :n[k]])
        np.testing.assert_array_equal(corners[k, :n[k]].cpu().numpy(), mc)
        np.testing.assert_array_equal(sums[k, :n[k]].cpu().numpy().view(np.uint32), ms)
        np.testing.assert_array_equal(counts[k, :n[k]].cpu().numpy().view(np.uint32), mn)
        assert lum[k, :n[k]].tobytes() == ml.tobytes()
        assert n[k] > 20 and (ml > 0.4).all()


# ---- 8. the 3-D link against the reference's fixtures --------------------------------------------------------------------
FIXTURES = ["tracker_lum_cross.npz", "tracker_lum_births.npz"]
#: (capacity, max_det, fused): one launch per frame (k_frame), and the two-launch link of tables beyond k_frame's LDS
#: (k_link + k_track; max_det > 2456)
SHAPES = [(512, 512, True), (512, 4096, False)]


def _fixture_frames(g):
    doff = g["det_off"]
    for f in range(len(doff) - 1):
        yield g["det"][doff[f]:doff[f + 1]], g["det_info"][doff[f]:doff[f + 1]]


def _tracker(g, capacity, max_det, fused):
    from ysmr_amd.tracker import DeviceTracker
    trk = DeviceTracker(max_disappeared=float(g["max_disappeared"]), fps=float(g["fps"]), use_gsff=False, capacity=capacity,
                        max_det=max_det, dimensions=3)
    assert trk.fused == fused and not trk.batched
    return trk


def _check_rows(rows, g, f0, f1):
    off = g["off"]
    sl = slice(off[f0], off[f1])
    assert len(rows) == off[f1] - off[f0]
    np.testing.assert_array_equal(rows["frame"], np.repeat(np.arange(f0, f1), np.diff(off[f0:f1 + 1])))
    np.testing.assert_array_equal(rows["track_id"], g["ids"][sl])
    assert rows["x"].tobytes() == np.ascontiguousarray(g["xy"][sl, 0]).tobytes()
    assert rows["y"].tobytes() == np.ascontiguousarray(g["xy"][sl, 1]).tobytes()
    np.testing.assert_array_equal(rows["disappeared"], g["disappeared"][sl])
    for k, key in enumerate(("w", "h", "angle")):
        np.testing.assert_array_equal(rows[key], g["info"][sl, k].astype(np.float32))


@pytest.mark.parametrize("capacity,max_det,fused", SHAPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_update3_frame_by_frame_matches_the_reference(torch_cuda, name, capacity, max_det, fused):
    torch = torch_cuda
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    g = golden(name)
    trk = _tracker(g, capacity, max_det, fused)
    rows = torch.empty(capacity * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    claim = torch.empty(capacity, dtype=torch.int32, device="cuda")
    new = torch.empty(max_det, dtype=torch.int32, device="cuda")
    scal = torch.zeros(4, dtype=torch.int32, device="cuda")
    off, coff = g["off"], g["claim_off"]
    lk = M.Linker(float(g["max_disappeared"]))
    for f, (det, info) in enumerate(_fixture_frames(g)):
        m = len(det)
        host = np.zeros((max(m, 1), 5))
        host[:m, :2], host[:m, 2:] = det[:, :2], info
        third = np.zeros(max(m, 1))
        third[:m] = det[:, 2]
        trk.update(torch.from_numpy(host).cuda(), m=m, frame=f, rows=rows, n_rows=scal[0:1], claim=claim, n_before=scal[1:2],
                   new_cols=new, n_new=scal[2:3], third=torch.from_numpy(third).cuda())
        n_rows, n_before, n_new = (int(v) for v in scal[:3].cpu().numpy())
        _check_rows(rows_to_numpy(rows, n_rows), g, f, f + 1)
        want_claims, want_born = lk.update(det)
        assert n_before == len(want_claims) and list(claim[:n_before].cpu().numpy()) == want_claims, f"claims, frame {f}"
        assert [(r, c) for r, c in enumerate(want_claims) if c >= 0] == [tuple(p) for p in g["claims"][coff[f]:coff[f + 1]]]
        assert list(new[:n_new].cpu().numpy()) == want_born, f"new-id order, frame {f}"
        ids, xyz, gone = trk.peek()
        sl = slice(off[f], off[f + 1])
        assert list(ids) == list(g["ids"][sl]) and list(gone) == list(g["disappeared"][sl])
        assert xyz.shape == (len(ids), 3) and xyz.tobytes() == np.ascontiguousarray(g["xy"][sl]).tobytes(), f"positions, frame {f}"
        assert trk.info()[:2] == (len(ids), int(g["next_id"][f])) and trk.info()[2] == 0


@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("capacity,max_det,fused", SHAPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_run3_in_batches_matches_the_reference(torch_cuda, name, capacity, max_det, fused, batch):
    torch = torch_cuda
    from ysmr_amd import _lib
    from ysmr_amd.tracker import rows_to_numpy
    g = golden(name)
    trk = _tracker(g, capacity, max_det, fused)
    frames = list(_fixture_frames(g))
    n_frames = len(frames)
    assert np.array_equal(g["det"][:, :2].astype(np.float32).astype(np.float64), g["det"][:, :2]), "x, y must be float32 values"
    det = np.zeros((n_frames, max_det, 5), np.float32)
    third = np.full((n_frames, max_det), 7.0)            # (stale slots hold a plausible value: they must not be read)
    counts = np.zeros(n_frames, np.int32)
    for f, (d, info) in enumerate(frames):
        counts[f] = len(d)
        det[f, :len(d), :2], det[f, :len(d), 2:] = d[:, :2], info
        third[f, :len(d)] = d[:, 2]
        det[f, len(d):, :2] = d[0, :2] if len(d) else 0.0  # ... and a stale slot's position is some track's exact spot
    det_d, third_d, counts_d = torch.from_numpy(det).cuda(), torch.from_numpy(third).cuda(), torch.from_numpy(counts).cuda()
    total = int(g["off"][-1])
    rows = torch.empty((total + 8) * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    for f0 in range(0, n_frames, batch):
        f1 = min(f0 + batch, n_frames)
        trk.run(det_d[f0:f1], counts_d[f0:f1], f0, rows, n, third=third_d[f0:f1])
    torch.cuda.synchronize()
    assert int(n.item()) == total
    _check_rows(rows_to_numpy(rows, total), g, 0, n_frames)
    ids, xyz, gone = trk.peek()
    sl = slice(g["off"][-2], g["off"][-1])
    assert list(ids) == list(g["ids"][sl]) and xyz.tobytes() == np.ascontiguousarray(g["xy"][sl]).tobytes()
    assert trk.info() == (len(ids), int(g["next_id"][-1]), 0)
    # reset keeps the dimension: the same frames give the same table again
    trk.reset()
    n.zero_()
    trk.run(det_d[:min(batch, n_frames)], counts_d[:min(batch, n_frames)], 0, rows, n, third=third_d[:min(batch, n_frames)])
    torch.cuda.synchronize()
    _check_rows(rows_to_numpy(rows, int(n.item())), g, 0, min(batch, n_frames))


def test_dimension_rules_of_the_handle(torch_cuda):
    torch = torch_cuda
    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker
    L = _lib.lib()
    ERR_ARG, ERR_STATE = _lib.YSMR_ERR_ARG, _lib.YSMR_ERR_STATE
    st = _lib.stream_ptr("cuda:0")
    gsff = DeviceTracker(fps=30.0, capacity=768, max_det=2048)               # tracking.ini's defaults
    plain = DeviceTracker(fps=30.0, use_gsff=False, capacity=768, max_det=2048)
    assert gsff.batched and plain.batched                                     # a 2-D handle links a batch with one launch, as before
    assert L.ysmr_tracker_dimensions(gsff._handle, 3) == ERR_ARG              # the reference has no such mode
    assert L.ysmr_tracker_dimensions(plain._handle, 4) == ERR_ARG
    assert L.ysmr_tracker_dimensions(plain._handle, 2) == _lib.YSMR_OK and plain.batched
    det = torch.tensor([[5.0, 6.0, 1.0, 1.0, 0.0]], dtype=torch.float64, device="cuda")
    third = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    rows = torch.empty(768 * _lib.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    n64 = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.ones(1, dtype=torch.int32, device="cuda")
    det32 = torch.zeros(1, 2048, 5, dtype=torch.float32, device="cuda")
    third2 = torch.zeros(1, 2048, dtype=torch.float64, device="cuda")
    # the 3-D calls on a 2-D handle
    assert L.ysmr_tracker_update3(plain._handle, st, det.data_ptr(), 1, third.data_ptr(), 1, None, 0, None, None, None, None, None, None) == ERR_STATE
    assert L.ysmr_tracker_run3(plain._handle, st, det32.data_ptr(), third2.data_ptr(), cnt.data_ptr(), 1, 0, rows.data_ptr(), 768, n64.data_ptr()) == ERR_STATE
    assert L.ysmr_tracker_peek3(plain._handle, st, None, None, third2.data_ptr(), None, None) == ERR_STATE
    # three dimensions: not batched, and the 2-D calls fail
    assert L.ysmr_tracker_dimensions(plain._handle, 3) == _lib.YSMR_OK
    assert not plain.batched and plain.fused
    assert L.ysmr_tracker_update(plain._handle, st, det.data_ptr(), 1, 1, None, 0, None, None, None, None, None, None) == ERR_STATE
    assert L.ysmr_tracker_run(plain._handle, st, det32.data_ptr(), cnt.data_ptr(), 1, 0, rows.data_ptr(), 768, n64.data_ptr()) == ERR_STATE
    assert L.ysmr_tracker_update3(plain._handle, st, det.data_ptr(), 1, third.data_ptr(), 1, None, 0, None, None, None, None, None, None) == _lib.YSMR_OK
    torch.cuda.synchronize()
    # ... fixed with the first frame, freed by a reset (which keeps it)
    assert L.ysmr_tracker_dimensions(plain._handle, 2) == ERR_STATE
    assert b"first frame" in L.ysmr_last_error()
    plain.reset()
    assert not plain.batched
    assert L.ysmr_tracker_update3(plain._handle, st, det.data_ptr(), 1, third.data_ptr(), 1, None, 0, None, None, None, None, None, None) == _lib.YSMR_OK
    plain.reset()
    assert L.ysmr_tracker_dimensions(plain._handle, 2) == _lib.YSMR_OK and plain.batched
    # and on a 2-D handle that has linked a frame
    other = DeviceTracker(fps=30.0, use_gsff=False, capacity=64, max_det=64)
    other.update(det, m=1)
    assert L.ysmr_tracker_dimensions(other._handle, 3) == ERR_STATE
    with pytest.raises(ValueError):
        other.update(det, m=1, third=third)


# ---- 9. CentroidTracker(dimensions=3) ------------------------------------------------------------------------------------
def test_centroid_tracker_in_three_dimensions(torch_cuda):
    from ysmr_amd.tracker import CentroidTracker
    g = golden("tracker_lum_births.npz")
    ct = CentroidTracker(max_disappeared=float(g["max_disappeared"]), fps=float(g["fps"]), use_gsff=False, capacity=512,
                         max_det=512, dimensions=3)
    off, coff = g["off"], g["claim_off"]
    for f, (det, info) in enumerate(_fixture_frames(g)):
        rects = [((float(d[0]), float(d[1]), float(d[2])), (float(i[0]), float(i[1]), float(i[2]))) for d, i in zip(det, info)]
        objs, infos = ct.update(rects)
        sl = slice(off[f], off[f + 1])
        assert list(objs.keys()) == list(g["ids"][sl])
        got = np.array(list(objs.values())).reshape(-1, 3)
        assert all(v.shape == (3,) for v in objs.values()) and got.tobytes() == np.ascontiguousarray(g["xy"][sl]).tobytes()
        held = ct.objects
        assert list(held.keys()) == list(objs.keys()) and all(np.array_equal(held[k], objs[k]) for k in held)
        np.testing.assert_array_equal(np.array([list(infos[i]) for i in objs], dtype=float).reshape(-1, 3), g["info"][sl])
        assert list(ct.disappeared.values()) == list(g["disappeared"][sl]) and ct.nextObjectID == g["next_id"][f]
        assert sorted(ct.last_claims) == sorted(map(tuple, g["claims"][coff[f]:coff[f + 1]].tolist()))
        if f == 3:
            with pytest.raises(ValueError):
                ct.update([((1.0, 2.0), (1, 1, 0))])        # a 3-D tracker fed (x, y)


# ---- 10. end to end ----------------------------------------------------------------------------------------------------
def _settings(**kw):
    from ysmr_amd.helper_file import default_settings
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                            "minimal frame count": 40, "include luminosity in tracking calculation": True, "disable gsff": True})
    s.update(kw)
    return s


def _rows_from_table(df, ref):
    """The seven columns as device-style rows in emission order; 'disappeared' from the expected table (a matched
    one-pixel blob also has w = h = angle = 0)."""
    from ysmr_amd import _lib
    df = df.sort_values(["POSITION_T", "TRACK_ID"]).reset_index(drop=True)
    rows = np.zeros(len(df), _lib.ROW_DTYPE)
    rows["frame"], rows["track_id"] = df["POSITION_T"], df["TRACK_ID"]
    rows["x"], rows["y"] = df["POSITION_X"], df["POSITION_Y"]
    rows["w"], rows["h"], rows["angle"] = df["WIDTH"], df["HEIGHT"], df["DEGREES_ANGLE"]
    if len(ref) == len(rows):
        rows["disappeared"] = [r[7] for r in ref]
    return rows


@pytest.mark.parametrize("adt", [2.0, -1.0], ids=["adaptive", "mean-gray"])
def test_track_bacteria_with_luminosity(tmp_path, oracle, caplog, adt):
    from ysmr_amd.helper_file import get_data
    from ysmr_amd.track_eval import track_bacteria
    frames = C.crossing_clip()
    assert frames.shape == (72, 240, 320)
    # what the reference's loop makes of the clip -- and the two conditions without which the clip would show nothing
    ref, lk = C.expected_rows(oracle, frames, 30.0, dims=3, adt=adt)
    assert lk.min_gap >= 1e-9, f"the expected table hangs on a distance gap of {lk.min_gap}"
    ref_2d, _ = C.expected_rows(oracle, frames, 30.0, dims=2, adt=adt)
    assert C.tracks_differ(ref, ref_2d), "the third coordinate decides nothing on this clip"
    path = tmp_path / "pairs.npy"
    np.save(path, frames)
    res = track_bacteria(str(path), settings=_settings(**{"adaptive double threshold": adt}), result_folder=str(tmp_path),
                         batch=16, max_det=256, capacity=256)
    assert res is not None
    df, fps, h, w, csv_path = res
    assert (fps, h, w) == (30.0, 240, 320) and os.path.basename(csv_path) == "pairs_list.csv"
    seven = ["TRACK_ID", "POSITION_T", "POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE"]
    assert list(df.columns) == seven and open(csv_path).readline().strip() == ",".join(seven)
    want = [r[:7] for r in ref]
    compare_rows(_rows_from_table(df, ref), want)
    compare_rows(_rows_from_table(get_data(csv_path), ref), want)
    # with the GSFF on the mode still answers None, as the reference's tracker raises there
    with caplog.at_level(logging.CRITICAL, logger="ysmr"):
        assert track_bacteria(str(path), settings=_settings(**{"adaptive double threshold": adt, "disable gsff": False}),
                              result_folder=str(tmp_path / "gsff")) is None
    assert any("disable gsff" in r.getMessage() for r in caplog.records)
