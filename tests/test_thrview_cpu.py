"""The threshold view where there is no GPU: ``ysmr_thrview_batch_host`` -- the code that decides a pixel in csrc/thrview.hip's
kernel, run on host arrays -- against tests/thrview_model.py, byte for byte; what the entry refuses; the header, the binding
and the ABI number; the settings key's spellings and the file name."""
import functools
import os
import re

import numpy as np
import pytest

import thrview_model as T

from ysmr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, GAP = 0xA5, 12


@functools.lru_cache(maxsize=None)
def case(shape, channels):
    """Frames, cls, mask of one shape: made once, never modified."""
    n, h, w = shape
    rng = np.random.default_rng(1000 * w + 10 * h + channels)
    frames = rng.integers(0, 256, shape if channels == 1 else shape + (3,), dtype=np.uint8)
    cls, mask = T.random_maps(rng, shape)
    for a in (frames, cls, mask):
        a.setflags(write=False)
    return frames, cls, mask


def host(frames, cls, mask, mode, bottom_up, stride=None, frame_bytes=None, channels=None, fill=FILL):
    n, h, w = cls.shape
    channels = (1 if frames.ndim == 3 else 3) if channels is None else channels
    stride = (3 * w + 3) & ~3 if stride is None else stride
    frame_bytes = stride * h if frame_bytes is None else frame_bytes
    out = np.full((n, frame_bytes), fill, np.uint8)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data      # noqa: E731
    keep = [np.ascontiguousarray(a) for a in (frames, cls, mask) if a is not None]  # noqa: F841 -- alive during the call
    rc = _lib.lib().ysmr_thrview_batch_host(ptr(frames), ptr(cls), ptr(mask), n, h, w, channels, mode, out.ctypes.data, stride, frame_bytes,
                                            bottom_up)
    _lib.check(rc, "ysmr_thrview_batch_host")
    return out


def test_all_eight_combinations_of_class_bits_and_mask_occur():
    seen = set()
    for shape in T.SHAPES:
        _, cls, mask = case(shape, 1)
        here = T.combinations(cls, mask)
        if cls.size >= 64:
            assert len(here) == 8, shape
        seen |= here
        assert set(np.unique(mask)) <= {0, 255} and cls.max() <= 7
    assert seen == {(c, k) for c in range(4) for k in (False, True)}
    assert max(int(case(s, 1)[1].max()) for s in T.SHAPES) > 3          # bits above the two the rule looks at are set somewhere


@pytest.mark.parametrize("bottom_up", [0, 1])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("mode", sorted(T.MODES))
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_export_stores_what_the_model_paints(shape, mode, channels, bottom_up):
    frames, cls, mask = case(shape, channels)
    n, h, w = shape
    code = T.MODES[mode]
    tight = (3 * w + 3) & ~3
    for stride, gap in ((tight, 0), (tight + 8, GAP)):           # ... and a stride larger than needed with a gap between frames
        want = T.stored(frames, cls, mask, code, stride, bottom_up, stride * h + gap, fill=FILL)
        got = host(frames, cls, mask, code, bottom_up, stride, stride * h + gap)
        assert np.array_equal(got, want), "{} bytes differ".format(int((got != want).sum()))
        rows = got[:, :stride * h].reshape(n, h, stride)
        assert (rows[:, :, 3 * w:] == 0).all() and (got[:, stride * h:] == FILL).all()


def test_pointers_a_mode_does_not_read_may_be_null():
    frames, cls, mask = case((2, 4, 63), 1)
    assert np.array_equal(host(None, cls, mask, T.MASK, 0, channels=1), T.stored(None, cls, mask, T.MASK))
    assert np.array_equal(host(None, cls, None, T.MARKERS, 1, channels=3), T.stored(None, cls, None, T.MARKERS, bottom_up=1))


def test_the_classes_picture_is_the_frame_where_nothing_is_painted():
    frames, cls, mask = case((1, 7, 67), 3)
    got = T.paint(frames, cls, mask, T.CLASSES)
    free = (mask == 0) & (cls & 1 == 0)
    assert free.any() and np.array_equal(got[free], frames[free])
    assert (got[(mask != 0) & (cls & 2 != 0)] == T.KEPT_MARKER).all() and (got[(mask != 0) & (cls & 2 == 0)] == T.KEPT).all()
    assert (got[(mask == 0) & (cls & 1 != 0)] == T.DROPPED).all()


def test_every_refused_argument_answers_err_arg_with_a_message_and_writes_nothing():
    frames, cls, mask = (np.ascontiguousarray(a) for a in case((3, 3, 5), 1))
    L = _lib.lib()
    n, h, w = cls.shape
    out = np.full((n, 16 * h), FILL, np.uint8)

    def call(**kw):
        a = dict(frames=frames.ctypes.data, cls=cls.ctypes.data, mask=mask.ctypes.data, n=n, h=h, w=w, channels=1, mode=2,
                 out=out.ctypes.data, stride=16, fb=16 * h)
        a.update(kw)
        return L.ysmr_thrview_batch_host(a["frames"], a["cls"], a["mask"], a["n"], a["h"], a["w"], a["channels"], a["mode"], a["out"],
                                         a["stride"], a["fb"], 0)

    assert call() == _lib.YSMR_OK
    out[:] = FILL
    refused = {"cls": dict(cls=None), "out": dict(out=None), "mask, mode 0": dict(mask=None, mode=0), "mask, mode 2": dict(mask=None),
               "frames": dict(frames=None), "channels 2": dict(channels=2), "channels 0": dict(channels=0), "channels 4": dict(channels=4),
               "mode 3": dict(mode=3), "mode -1": dict(mode=-1), "stride below 3 W": dict(stride=12), "stride not a multiple of 4": dict(stride=18, fb=18 * h),
               "frame bytes too small": dict(fb=16 * h - 4), "frame bytes not a multiple of 4": dict(fb=16 * h + 2),
               "output not aligned": dict(out=out.ctypes.data + 1), "no frames": dict(n=0), "no rows": dict(h=0), "no columns": dict(w=0)}
    for what, kw in refused.items():
        assert call(**kw) == _lib.YSMR_ERR_ARG, what
        message = L.ysmr_last_error().decode()
        assert message.startswith("thrview: ") and len(message) > 20, what
        assert (out == FILL).all(), what
    assert call(mask=None, mode=1) == _lib.YSMR_OK and call(frames=None, mode=0) == _lib.YSMR_OK


def test_the_header_declares_the_exports_the_binding_binds_them_and_the_abi_is_15():
    header = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    L = _lib.lib()
    for name in ("ysmr_thrview_batch", "ysmr_thrview_batch_host"):
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes
    assert len(L.ysmr_thrview_batch.argtypes) == 13 and len(L.ysmr_thrview_batch_host.argtypes) == 12
    assert re.search(r"#define\s+YSMR_ABI_VERSION\s+15\b", header) and _lib.ABI_VERSION == 15 and L.ysmr_abi_version() == 15


def test_the_settings_keys_spellings():
    from ysmr_amd.track_eval import threshold_view_mode
    for absent in ({}, {"hip save threshold video": False}, {"hip save threshold video": None}, {"hip save threshold video": ""},
                   {"hip save threshold video": "False"}, {"hip save threshold video": "no"}, {"hip save threshold video": 0}):
        assert threshold_view_mode(absent) is None
    for value, mode in ((True, 0), ("mask", 0), ("MASK", 0), (" Mask ", 0), ("True", 0), ("markers", 1), ("Markers", 1), ("MARKERS", 1),
                        ("classes", 2), ("Classes", 2), ("CLASSES", 2)):
        assert threshold_view_mode({"hip save threshold video": value}) == mode, value
    for bad in ("thresh", "marker", 2, 1.5, "mask,markers", ["mask"]):
        with pytest.raises(ValueError, match="hip save threshold video"):
            threshold_view_mode({"hip save threshold video": bad})


def test_the_key_in_a_tracking_ini_and_the_file_name(tmp_path):
    from ysmr_amd.helper_file import create_configs, default_settings, get_configs
    from ysmr_amd.track_eval import threshold_video_path, threshold_view_mode
    assert "hip save threshold video" not in default_settings()
    ini = tmp_path / "tracking.ini"
    create_configs(str(ini))
    assert "hip save threshold video" not in get_configs(str(ini))     # a tracking.ini without the key reads as before
    ini.write_text(ini.read_text().replace("[ADVANCED VIDEO SETTINGS]", "[ADVANCED VIDEO SETTINGS]\nhip save threshold video = Classes"))
    assert threshold_view_mode(get_configs(str(ini))) == 2
    ini.write_text(ini.read_text().replace("= Classes", "= True"))
    assert threshold_view_mode(get_configs(str(ini))) == 0
    s = default_settings()
    assert threshold_video_path("/data/run 3/clip.01.avi", str(tmp_path), s) == str(tmp_path / "clip.01_threshold_output.avi")
    assert threshold_video_path("/data/run 3/clip.01.avi", str(tmp_path)) == str(tmp_path / "clip.01_threshold_output.avi")


def test_markers_without_a_marker_threshold_is_one_warning_and_no_view(caplog):
    import logging
    from ysmr_amd.track_eval import _threshold_view_of
    logger = logging.getLogger("ysmr").getChild("test")
    with caplog.at_level(logging.WARNING, logger="ysmr"):
        assert _threshold_view_of({"hip save threshold video": "markers", "adaptive double threshold": 2.0}, logger) == 1
        assert caplog.text == ""
        for adt in (0, 0.0, -1, -1.0):
            caplog.clear()
            assert _threshold_view_of({"hip save threshold video": "Markers", "adaptive double threshold": adt}, logger) is None
            assert len(caplog.records) == 1 and caplog.records[0].levelno == logging.WARNING and "markers" in caplog.text
            for other in ("mask", "classes", True):
                assert _threshold_view_of({"hip save threshold video": other, "adaptive double threshold": adt}, logger) is not None
        assert _threshold_view_of({"adaptive double threshold": -1}, logger) is None
