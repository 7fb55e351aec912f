"""Luminosity as a third tracking coordinate: what can be checked without a GPU.

Tests 1-3 pin the test-side model (tests/luminosity_model.py) that the device results are judged by -- they would pass
without the feature and are here so that a wrong model cannot make a wrong kernel look right.  The rest exercises the
product: the kernel's own arithmetic run on the host (``ysmr_luminosity_batch_host`` shares the code that decides a
pixel with ``k_luminosity``), ``save_list(illumination=True)``, the kernel's resource figures and the argument rules
of the 3-D tracker classes.
"""
import logging
import os
import re
import subprocess

import numpy as np
import pytest

import luminosity_model as M
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_rects(rng, n, H, W):
    """Sizes including 0 and 1, angles 0 / 90 / -90 / arbitrary, centres inside, on and beyond the border."""
    out = []
    for _ in range(n):
        kind = rng.integers(0, 4)
        if kind == 0:
            cx, cy = rng.uniform(3, W - 3), rng.uniform(3, H - 3)
        elif kind == 1:      # on the border
            cx, cy = rng.choice([0.0, W - 1.0, rng.uniform(0, W)]), rng.choice([0.0, H - 1.0, rng.uniform(0, H)])
        else:                # up to three pixels beyond it
            cx, cy = rng.uniform(-3, W + 3), rng.uniform(-3, H + 3)
        w = rng.choice([0, 1, 2, 3.5, 7, 12.3, 20, rng.uniform(0, 30)])
        h = rng.choice([0, 1, 2.2, 4, 9, rng.uniform(0, 30)])
        ang = rng.choice([0, 90, -90, rng.uniform(-90, 90)])
        out.append((cx, cy, w, h, ang))
    return np.array(out, np.float32)


# ---- 1. the fill model against an independent formulation ----------------------------------------------------------------
def test_fill_model_against_exact_geometry():
    rng = np.random.default_rng(3)
    H = W = 64
    rects = random_rects(rng, 2500, H, W)
    missing = far = 0
    for det in rects:
        pts = M.int_corners(det)
        f = M.fill(pts, H, W)
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        for y in range(max(min(ys), 0), min(max(ys), H - 1) + 1):
            for x in range(max(min(xs), 0), min(max(xs), W - 1) + 1):
                if M.inside_strict(pts, x, y) and (x, y) not in f:
                    missing += 1
        for (x, y) in f:
            assert 0 <= x < W and 0 <= y < H
            if M.dist2_to_quad(pts, x, y) > 1.0 + 1e-9:
                far += 1
        # a box whose four corners lie beyond the same side of the frame fills nothing
        if max(xs) < 0 or min(xs) >= W or max(ys) < 0 or min(ys) >= H:
            assert not f
    assert missing == 0, f"{missing} pixels strictly inside a quadrilateral are not filled"
    assert far == 0, f"{far} filled pixels lie farther than 1 px from their quadrilateral"


def test_fill_model_of_a_single_pixel_and_of_boxes_outside():
    H, W = 20, 30
    for (cx, cy) in [(0.0, 0.0), (7.0, 3.0), (29.0, 19.0), (12.5, 8.5)]:
        for ang in (0.0, 90.0, -90.0, 37.0):
            pts = M.int_corners([cx, cy, 0.0, 0.0, ang])
            assert M.fill(pts, H, W) == {(int(cx), int(cy))}
    for det in [(-9.0, 5.0, 4.0, 3.0, 20.0), (40.0, 5.0, 6.0, 2.0, 0.0), (5.0, -8.0, 3.0, 3.0, 90.0), (5.0, 31.0, 5.0, 4.0, 61.0)]:
        assert M.fill(M.int_corners(det), H, W) == set()
    # partly outside: what is inside is filled
    pts = M.int_corners([0.0, 0.0, 6.0, 4.0, 0.0])
    assert M.fill(pts, H, W) == {(x, y) for x in range(0, 4) for y in range(0, 3)}


# ---- 2. ... and against cv2 where there is one -----------------------------------------------------------------------------
def test_cv2_cross_check_if_available():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(5)
    H, W = 48, 64
    gray = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for det in random_rects(rng, 600, H, W):
        rect = ((float(det[0]), float(det[1])), (float(det[2]), float(det[3])), float(det[4]))
        box = np.intp(cv2.boxPoints(rect))
        pts, total, count, lum = M.luminosity(gray, det)
        assert [tuple(int(v) for v in p) for p in box] == pts
        mask = np.zeros((H, W), np.uint8)
        cv2.fillPoly(mask, [box], 255)
        assert {(int(x), int(y)) for y, x in zip(*np.nonzero(mask))} == M.fill(pts, H, W)
        assert cv2.mean(gray, mask)[0] / 100 == lum


# ---- 3. the model linker against the reference's own tracker ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["tracker_lum_cross.npz", "tracker_lum_births.npz"])
def test_model_linker_reproduces_the_reference_fixture(name):
    g = golden(name)
    assert g["det"].shape[1] == 3 and g["xy"].shape[1] == 3 and not bool(g["use_gsff"])
    lk = M.Linker(float(g["max_disappeared"]))
    off, doff, coff = g["off"], g["det_off"], g["claim_off"]
    for f in range(len(off) - 1):
        claims, _ = lk.update(g["det"][doff[f]:doff[f + 1]])
        ids = list(lk.objects.keys())
        assert ids == list(g["ids"][off[f]:off[f + 1]])
        assert [lk.disappeared[i] for i in ids] == list(g["disappeared"][off[f]:off[f + 1]])
        assert [(r, c) for r, c in enumerate(claims) if c >= 0] == [tuple(p) for p in g["claims"][coff[f]:coff[f + 1]]]
        assert lk.next_id == int(g["next_id"][f])
        xy = np.array([lk.objects[i] for i in ids]).reshape(-1, 3)
        assert xy.tobytes() == g["xy"][off[f]:off[f + 1]].tobytes()       # bit for bit
    assert lk.min_gap > 0.0


# ---- the kernel's arithmetic, run on the host, against the model ------------------------------------------------------------
def _host_luminosity(frames, det, counts, cv_flavour=0):
    from ysmr_amd import _lib
    B, md = det.shape[:2]
    ch = 1 if frames.ndim == 3 else 3
    frames = np.ascontiguousarray(frames)
    det = np.ascontiguousarray(det, np.float32)
    counts = np.ascontiguousarray(counts, np.int32)
    lum = np.full((B, md), -1.0)
    total = np.full((B, md), 0xFFFFFFFF, np.uint32)
    count = np.full((B, md), 0xFFFFFFFF, np.uint32)
    corners = np.full((B, md, 4, 2), -7, np.int32)
    rc = _lib.lib().ysmr_luminosity_batch_host(frames.ctypes.data, B, frames.shape[1], frames.shape[2], ch, det.ctypes.data,
                                               counts.ctypes.data, md, cv_flavour, lum.ctypes.data, total.ctypes.data,
                                               count.ctypes.data, corners.ctypes.data)
    _lib.check(rc, "ysmr_luminosity_batch_host")
    return corners, total, count, lum


@pytest.mark.parametrize("H,W,ch,flavour", [(64, 64, 1, 0), (37, 61, 1, 0), (40, 50, 3, 0), (33, 47, 3, 2)])
def test_kernel_arithmetic_on_the_host_equals_the_model(H, W, ch, flavour):
    """Every row of a filled box is ONE run [lo, hi] in the kernel, worked out in closed form; the model draws lines and
    spans pixel by pixel into a set.  Integers equal for every box, the value equal as a double; slots past a frame's count
    are not written."""
    rng = np.random.default_rng(H * 1000 + W)
    B, md = 3, 300
    frames = rng.integers(0, 256, (B, H, W) + ((3,) if ch == 3 else ()), dtype=np.uint8)
    det = np.stack([random_rects(rng, md, H, W) for _ in range(B)])
    det[0, :4, 2:4] = [[200, 3], [3, 150], [90, 90], [0, 0]]      # longer than the frame; a whole-frame island; a pixel
    counts = np.array([md, 0, md - 11], np.int32)
    corners, total, count, lum = _host_luminosity(frames, det, counts, flavour)
    for b in range(B):
        n = counts[b]
        gray = frames[b] if ch == 1 else M.bgr2gray(frames[b], gray_3x=bool(flavour & 2))
        mc, ms, mn, ml = M.luminosity_frame(gray, det[b, :n])
        np.testing.assert_array_equal(corners[b, :n], mc)
        np.testing.assert_array_equal(count[b, :n], mn)
        np.testing.assert_array_equal(total[b, :n], ms)
        assert lum[b, :n].tobytes() == ml.tobytes()
        assert (lum[b, n:] == -1.0).all() and (count[b, n:] == 0xFFFFFFFF).all() and (corners[b, n:] == -7).all()


def test_luminosity_argument_checks():
    from ysmr_amd import _lib
    L = _lib.lib()
    f = np.zeros((1, 8, 8), np.uint8)
    d = np.zeros((1, 4, 5), np.float32)
    c = np.zeros(1, np.int32)
    out = np.zeros((1, 4))
    args = lambda ch=1, md=4, lum=out.ctypes.data: (f.ctypes.data, 1, 8, 8, ch, d.ctypes.data, c.ctypes.data, md, 0, lum, None, None, None)  # noqa: E731
    assert L.ysmr_luminosity_batch_host(*args()) == _lib.YSMR_OK
    assert L.ysmr_luminosity_batch_host(*args(ch=2)) == _lib.YSMR_ERR_ARG
    assert L.ysmr_luminosity_batch_host(*args(md=0)) == _lib.YSMR_ERR_ARG
    assert L.ysmr_luminosity_batch_host(*args(lum=None)) == _lib.YSMR_ERR_ARG


# ---- 4. save_list(illumination=True) ------------------------------------------------------------------------------------
def test_save_list_with_illumination_writes_the_eighth_column(tmp_path):
    from ysmr_amd.helper_file import save_list
    old, path = save_list(str(tmp_path / "clip.avi"), result_folder=str(tmp_path), first_call=True, illumination=True)
    assert old is False and path == str(tmp_path / "clip_list.csv")
    coords = [(0, 0, (1.5, 2.25, 0.8123), (3.0, 4.5, -45.0)),
              (0, 1.0, (np.float64(10.1), np.float64(0.1) + np.float64(0.2), np.float64(1.7) / 3), (0, 0, 0)),
              (12, 7, (100.0, 200.0, 2.0), (np.float32(2.5), np.float32(1.0), np.float32(-90.0)))]
    assert save_list(path, coords=coords, illumination=True) == (None, None)
    assert save_list(path, coords=coords[:1], illumination=True) == (None, None)
    expected = ("TRACK_ID,POSITION_T,POSITION_X,POSITION_Y,WIDTH,HEIGHT,DEGREES_ANGLE,ILLUMINATION\n"
                "0,0,1.5,2.25,3.0,4.5,-45.0,0.8123\n"
                "1,0,10.1,0.30000000000000004,0,0,0,0.5666666666666667\n"
                "7,12,100.0,200.0,2.5,1.0,-90.0,2.0\n"
                "0,0,1.5,2.25,3.0,4.5,-45.0,0.8123\n")
    with open(path, "rb") as fh:
        assert fh.read() == expected.encode()
    # the default is what it was: seven columns, and a third coordinate is ignored
    old, path2 = save_list(str(tmp_path / "other.avi"), result_folder=str(tmp_path), first_call=True)
    save_list(path2, coords=coords[:1])
    with open(path2, "rb") as fh:
        assert fh.read() == b"TRACK_ID,POSITION_T,POSITION_X,POSITION_Y,WIDTH,HEIGHT,DEGREES_ANGLE\n0,0,1.5,2.25,3.0,4.5,-45.0\n"


# ---- 5. kernel resources ------------------------------------------------------------------------------------------------
def test_k_luminosity_needs_no_scratch(tmp_path):
    from test_kernel_resources import LIB, _gfx950_code_objects, _tool
    objcopy, readelf = _tool("llvm-objcopy"), _tool("llvm-readelf")
    assert os.path.exists(LIB), "libysmr_hip.so is not built"
    if not objcopy or not readelf:
        pytest.skip("llvm-objcopy / llvm-readelf not found")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "host.so")], check=True, capture_output=True)
    found = []
    for k, co in enumerate(_gfx950_code_objects(fat.read_bytes())):
        path = tmp_path / f"co{k}.o"
        path.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            m = re.search(r"^\s*\.?name:\s+(\S*k_luminosity\S*)\s*$", block, re.M)
            if m:
                field = lambda name: int(re.search(r"\.?" + name + r":\s+(\d+)", block).group(1))  # noqa: E731
                found.append(m.group(1))
                assert field("vgpr_spill_count") == 0, m.group(1)
                assert field("private_segment_fixed_size") == 0, m.group(1)
    assert len(found) == 2, f"expected the gray and the BGR instantiation of k_luminosity, found {found}"


# ---- 6. argument rules that need no GPU call ----------------------------------------------------------------------------
def test_three_dimensions_need_the_filter_bank_off():
    from ysmr_amd.tracker import CentroidTracker, DeviceTracker
    with pytest.raises(ValueError, match="use_gsff=False"):
        DeviceTracker(dimensions=3)                      # use_gsff defaults to True
    with pytest.raises(ValueError, match="use_gsff=False"):
        CentroidTracker(dimensions=3, use_gsff=True)
    with pytest.raises(ValueError, match="2 or 3"):
        DeviceTracker(dimensions=4, use_gsff=False)


def test_track_bacteria_with_luminosity_and_gsff_still_returns_none(tmp_path, caplog):
    from ysmr_amd.helper_file import default_settings
    from ysmr_amd.track_eval import track_bacteria
    clip = tmp_path / "clip.npy"
    np.save(clip, np.zeros((10, 8, 8), np.uint8))
    s = default_settings(**{"user input": False, "select files": False, "display video analysis": False, "log to file": False,
                            "include luminosity in tracking calculation": True, "minimal frame count": 5})
    assert not s["disable gsff"]
    with caplog.at_level(logging.CRITICAL, logger="ysmr"):
        assert track_bacteria(str(clip), settings=s, result_folder=str(tmp_path)) is None
    assert any("disable gsff" in r.getMessage() and "reference" in r.getMessage() for r in caplog.records)
