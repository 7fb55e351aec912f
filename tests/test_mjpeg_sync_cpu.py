"""The synchronising Motion-JPEG entropy decode without a GPU: its model (tests/jpeg_sync_model.py) against the serial decoder of
tests/jpeg_decode_model.py -- coefficients and status, for every subsequence size and pass width of the list, 2 and 4 bytes
among them, where whole subsequences hold no symbol start -- and the host side of the three entry points of the C ABI."""
import ctypes
import functools
import os

import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_sync_model as sm
import mjpeg_sync_streams as ms
from test_mjpeg_decode_cpu import fixture

SUBSEQUENCE_BYTES = (2, 4, 16, 128)
PER_PASS = (2, 64)


@functools.lru_cache(maxsize=None)
def serial(stream, height, width, sampling):
    """(status, planes or None) of the serial decoder."""
    try:
        _, tables, slots, ri, start = dm._headers(stream, height, width, sampling)
        return 0, dm._coefficients(stream, height, width, sampling, tables, slots, ri, start)
    except dm._Flag as flag:
        return flag.status, None


def restartless():
    """The fixture's streams whose first (only) frame has no DRI, the flagged ones among them."""
    out = []
    for e, stream, _ in fixture():
        try:
            if dm._headers(stream, e["height"], e["width"], e["sampling"])[3]:
                continue
        except dm._Flag:
            pass
        out.append(e["name"])
    return out


def agree(stream, height, width, sampling, sub, per_pass):
    want_status, want = serial(stream, height, width, sampling)
    planes, status, rounds = sm.decode(stream, height, width, sampling, sub, per_pass)
    assert status == want_status
    if status == 0:
        for c, plane in enumerate(want):
            np.testing.assert_array_equal(planes[c], plane, err_msg="component {}".format(c))
    assert all(1 <= r <= per_pass for r in rounds)
    return rounds


def test_the_fixture_has_restartless_streams_of_every_kind():
    found = restartless()
    assert len(found) >= 20 and "444_cut_in_half_23x41" in found and "444_progressive_23x41" in found
    assert {n.split("_")[0] for n in found} == {"L", "444", "422", "420"}


@pytest.mark.parametrize("per_pass", PER_PASS)
@pytest.mark.parametrize("sub", SUBSEQUENCE_BYTES)
def test_the_model_equals_the_serial_decoder_on_the_fixture(sub, per_pass):
    names = restartless()
    for e, stream, _ in fixture():
        if e["name"] in names:
            agree(stream, e["height"], e["width"], e["sampling"], sub, per_pass)
            assert serial(stream, e["height"], e["width"], e["sampling"])[0] == e["status"]


@pytest.mark.parametrize("per_pass", PER_PASS)
@pytest.mark.parametrize("sub", SUBSEQUENCE_BYTES)
def test_the_all_zero_frame_takes_as_many_rounds_as_a_pass_has_lanes(sub, per_pass):
    """Six bits per block for ever: a lane that starts off the boundaries stays off them, and only the true state, handed on
    a lane per round, puts it right.  (A lane whose first bit happens to be a boundary is right from the start, so the last
    lanes of a pass may be: one round less.)"""
    stream, h, w, s = ms.zeros(40, 40)
    rounds = agree(stream, h, w, s, sub, per_pass)
    lanes = min(per_pass, ms.subsequences(stream, sub))
    assert max(rounds) >= lanes - 1
    if sub in (2, 4) or per_pass == 2:
        assert max(rounds) == per_pass


@pytest.mark.parametrize("per_pass", PER_PASS)
@pytest.mark.parametrize("sub", SUBSEQUENCE_BYTES)
def test_long_symbols_and_stuffing(sub, per_pass):
    stream, h, w, s = ms.dense()
    assert stream.count(b"\xff\x00") >= 50
    agree(stream, h, w, s, sub, per_pass)


@pytest.mark.parametrize("per_pass", PER_PASS)
@pytest.mark.parametrize("sub", SUBSEQUENCE_BYTES)
def test_the_dc_prediction_passes_16_bits(sub, per_pass):
    stream, h, w, s = ms.dc_wrap()
    assert max(int(p[..., 0].max()) for p in serial(stream, h, w, s)[1]) > 32767
    agree(stream, h, w, s, sub, per_pass)


@pytest.mark.parametrize("sampling", (0, 1, 2, 3))
def test_noise_of_every_sampling(sampling):
    """(the luminance's scan order is not its plane order for 4:2:2 and 4:2:0: the DC sums follow the scan)"""
    stream, h, w, s = ms.noise(37, 45, sampling)
    for sub, per_pass in ((4, 64), (16, 2), (128, 64)):
        agree(stream, h, w, s, sub, per_pass)


def test_damaged_streams_get_the_serial_decoders_status():
    stream, h, w, s = ms.noise(37, 45, 3)
    at = stream.index(b"\xff\xda") + 14
    middle = (at + len(stream)) // 2
    for damaged in (stream[:middle], stream[:middle] + b"\xff\xd9" + stream[middle:], stream[:middle] + b"\xff\xd0" + stream[middle:],
                    stream[:at + 40] + b"\x5a" + stream[at + 41:], stream[:-2]):
        for sub, per_pass in ((4, 64), (16, 2), (128, 64)):
            agree(damaged, h, w, s, sub, per_pass)
    assert serial(stream[:middle], h, w, s)[0] == dm.CORRUPT


def test_a_stream_with_a_restart_interval_is_not_this_models():
    e, stream, _ = next(item for item in fixture() if item[0]["name"] == "L_rows_23x41_q50_saturated")
    with pytest.raises(ValueError):
        sm.decode(stream, e["height"], e["width"], e["sampling"], 16, 64)


# ---- the C ABI (host side) --------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_three_entry_points():
    from ysmr_amd import _lib
    L = _lib.lib()
    for name in ("ysmr_mjpeg_decode_sync_workspace_bytes", "ysmr_mjpeg_decode_batch_sync", "ysmr_mjpeg_decode_sync_geometry"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "ysmr_hip.h")).read()
    for name in ("ysmr_mjpeg_decode_sync_workspace_bytes(", "ysmr_mjpeg_decode_batch_sync(", "ysmr_mjpeg_decode_sync_geometry("):
        assert name in header


def geometry():
    from ysmr_amd import _lib
    sub, per_pass = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.lib().ysmr_mjpeg_decode_sync_geometry(ctypes.byref(sub), ctypes.byref(per_pass))
    return sub.value, per_pass.value


def test_the_geometry_is_positive():
    from ysmr_amd import _lib
    sub, per_pass = geometry()
    assert sub > 0 and per_pass > 0
    _lib.lib().ysmr_mjpeg_decode_sync_geometry(None, None)                 # (either pointer may be NULL)


def test_the_workspace_function():
    from ysmr_amd import _lib
    L = _lib.lib()
    new, old = L.ysmr_mjpeg_decode_sync_workspace_bytes, L.ysmr_mjpeg_decode_workspace_bytes
    for bad in ((1, 8, 8, 3, 4), (1, 8, 8, 3, -1), (1, 8, 8, 3, 0), (1, 8, 8, 1, 2), (0, 8, 8, 1, 0), (-1, 8, 8, 1, 0), (1, 0, 8, 1, 0),
                (1, 8, 65536, 1, 0), (1, 65536, 8, 1, 0)):
        assert old(*bad) == 0 and new(*bad, 4096) == 0, bad
    for chunk in (0, -1, -2 ** 31, 2 ** 27):
        assert new(1, 8, 8, 1, 0, chunk) == 0, chunk
    for shape in ((1, 8, 8, 1, 0), (248, 922, 1228, 1, 0), (3, 23, 41, 3, 1), (65, 31, 33, 3, 2), (7, 65535, 65535, 3, 3)):
        sizes = [new(*shape, chunk) for chunk in (1, 300, 600, 4096, 136992, 2 ** 27 - 1)]
        assert sizes[0] > old(*shape) > 0, shape
        assert sizes == sorted(sizes) and sizes[1] < sizes[2] < sizes[3] < sizes[4] < sizes[5], shape
        assert all(size % 256 == 0 for size in sizes)
        # the entropy data without its stuffing has a place of its own for every frame
        assert sizes[4] - old(*shape) >= shape[0] * 136992
    # a total that no size_t holds is refused, not wrapped
    assert new(2 ** 31 - 1, 65535, 65535, 3, 3, 2 ** 27 - 1) == 0
