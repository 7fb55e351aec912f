"""The figures' PNG files on the device (csrc/png.hip): ``ysmr_png_deflate`` against tests/png_deflate_model.py byte for
byte and against zlib, ``ysmr_plot_stamp`` against the host's ``stamp_text`` / ``stamp_text_vertical``, and every figure of
``evaluate_tracks`` with and without 'hip png on device'."""
import os
import zlib

import numpy as np
import pytest

import png_deflate_model as pm
import png_tools

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _deflate(rgb):
    import torch
    from ysmr_amd import plot_functions as pf
    return pf.device_deflate(torch.from_numpy(np.array(rgb)).to(DEV))


# ---- deflate ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", pm.CASE_IDS)
def test_stream_is_the_models_byte_for_byte(case_id):
    from ysmr_amd import _lib
    rgb, want = pm.case(case_id)
    got = _deflate(rgb)
    h, w = rgb.shape[:2]
    assert len(got) <= _lib.lib().ysmr_png_stream_bytes_max(w, h)
    assert zlib.decompress(got) == pm.scanlines(rgb).tobytes()
    assert len(got) == len(want), "{} bytes, the model has {}".format(len(got), len(want))
    diff = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert not len(diff), "{} bytes differ, the first at {}".format(len(diff), diff[0])


def test_random_literals_fit_the_bound_and_come_close():
    from ysmr_amd import _lib
    rgb, _ = pm.case("random144-341x67")
    got = _deflate(rgb)
    bound = pm.stream_bytes_bound(341, 67)
    assert 0.98 * bound <= len(got) <= bound <= _lib.lib().ysmr_png_stream_bytes_max(341, 67)


def test_full_size_canvas_twice():
    """3507 x 2480 with 3000 discs: decompresses to the scanline bytes, two runs give identical bytes."""
    import torch
    from ysmr_amd import plot_functions as pf
    rgb = pm.discs_canvas()
    dev = torch.from_numpy(rgb).to(DEV)
    first, second = pf.device_deflate(dev), pf.device_deflate(dev)
    assert first == second
    raw = pm.scanlines(rgb).tobytes()
    assert zlib.decompress(first) == raw
    assert first[:2] == b"\x78\x01" and int.from_bytes(first[-4:], "big") == zlib.adler32(raw) & 0xFFFFFFFF
    assert len(first) < len(raw) // 10                                        # mostly white: the matches are found


def test_write_png_device_lays_the_file_out_as_write_png(tmp_path):
    import torch
    from ysmr_amd import plot_functions as pf
    rgb, _ = pm.case("periods-341x67")
    pf.write_png(str(tmp_path / "host.png"), rgb, 150)
    pf.write_png_device(str(tmp_path / "device.png"), torch.from_numpy(np.array(rgb)).to(DEV), 150)
    host, hc = png_tools.read_png(str(tmp_path / "host.png"))
    dev, dc = png_tools.read_png(str(tmp_path / "device.png"))
    assert np.array_equal(host, rgb) and np.array_equal(dev, rgb)
    assert hc["order"] == dc["order"] == [b"IHDR", b"pHYs", b"IDAT", b"IEND"]
    assert hc[b"IHDR"] == dc[b"IHDR"] and hc[b"pHYs"] == dc[b"pHYs"]


def test_short_buffers_are_refused():
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    w, h = 85, 2
    rgb = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.ysmr_png_workspace_bytes(w, h), dtype=torch.uint8, device=DEV)
    out = torch.empty(L.ysmr_png_stream_bytes_max(w, h), dtype=torch.uint8, device=DEV)
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    call = lambda ws_bytes, out_bytes: L.ysmr_png_deflate(_lib.stream_ptr(DEV), rgb.data_ptr(), w, h, ws.data_ptr(), ws_bytes, out.data_ptr(),
                                                          out_bytes, n.data_ptr())
    assert call(ws.numel() - 1, out.numel()) == _lib.YSMR_ERR_ARG
    assert call(ws.numel(), out.numel() - 1) == _lib.YSMR_ERR_ARG
    assert call(ws.numel(), out.numel()) == _lib.YSMR_OK
    assert zlib.decompress(out[:int(n.item())].cpu().numpy().tobytes()) == bytes(h * (1 + 3 * w))


# ---- the lettering ---------------------------------------------------------------------------------------------------

def _stamp_both(shape, calls, background=200):
    """``calls``: (function name, args, kwargs) of plot_functions, applied to a NumPy canvas and, recorded, by the device."""
    import torch
    from ysmr_amd import plot_functions as pf
    want = np.full(shape, background, np.uint8)
    stamps = pf.StampList(shape[0], shape[1])
    for name, args, kwargs in calls:
        getattr(pf, name)(want, *args, **kwargs)
        getattr(pf, name)(stamps, *args, **kwargs)
    dev = torch.full(shape, background, dtype=torch.uint8, device=DEV)
    pf.device_stamp(dev, stamps)
    got = dev.cpu().numpy()
    assert np.array_equal(got, want), "{} pixels differ".format((got != want).any(axis=2).sum())
    return want, stamps


def test_stamp_scales_edges_and_outside():
    H, W = 90, 160
    calls = [("stamp_text", (5 + 3 * s, 2 + 9 * s * (s - 1) // 2, "Ag{}µ".format(s), s), dict(colour=(10 * s, 20, 30))) for s in (1, 2, 3, 4)]
    calls += [("stamp_text", (-7, 40, "left", 2), {}),                        # clipped at each of the four edges
              ("stamp_text", (W - 9, 60, "right", 2), dict(colour=(255, 0, 0))),
              ("stamp_text", (70, -5, "top", 2), dict(colour=(0, 255, 0))),
              ("stamp_text", (70, H - 6, "bottom", 2), dict(colour=(0, 0, 255))),
              ("stamp_text", (W, 10, "centre", 3), dict(anchor="centre")),
              ("stamp_text", (3, 75, "ending", 1), dict(anchor="right")),
              ("stamp_text_vertical", (-4, 45, "up", 3), dict(colour=(9, 9, 9))),
              ("stamp_text_vertical", (W - 5, 5, "up", 2), {}),
              ("stamp_text_vertical", (100, H, "up", 2), {}),
              ("stamp_text", (W, 10, "out", 2), {}),                          # wholly outside, every side
              ("stamp_text", (-200, 10, "out", 2), {}),
              ("stamp_text", (10, H, "out", 2), {}),
              ("stamp_text", (10, -14, "out", 2), {}),
              ("stamp_text_vertical", (W + 3, 10, "out", 1), {}),
              ("stamp_text", (10, 10, "", 2), {})]
    want, stamps = _stamp_both((H, W, 3), calls)
    assert len(stamps.records) == len(calls) - 1 and (want != 200).any()      # (the empty text has no bitmap)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_overlapping_stamps_the_later_one_wins(order):
    pair = [("stamp_text", (4, 4, "####", 3), dict(colour=(255, 0, 0))), ("stamp_text", (10, 9, "####", 3), dict(colour=(0, 0, 255)))]
    calls = [pair[order[0]], pair[order[1]]]
    want, _ = _stamp_both((48, 100, 3), calls)
    first, last = calls[0][2]["colour"], calls[1][2]["colour"]
    assert (want == last).all(axis=2).sum() > (want == first).all(axis=2).sum() > 0     # the earlier one is partly covered


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_evaluate_tracks_writes_the_same_figures_with_the_key(tmp_path):
    from select_tables import make_table, select_settings
    from ysmr_amd import evaluate_tracks
    df = make_table(5, n_tracks=25, max_len=500)
    size = df.groupby("TRACK_ID")["TRACK_ID"].transform("size")
    df = df[size >= 32].reset_index(drop=True)
    host = select_settings(**{"store generated statistical .csv file": True, "store final analysed .csv file": True,
                              "hip violin plots": True})
    assert host["save large plots"] and host["save rose plot"] and host["save angle distribution plot / bins"]
    assert "hip png on device" not in host
    device = dict(host, **{"hip png on device": True})
    for name, settings in (("host", host), ("device", device)):
        os.makedirs(tmp_path / name)
        evaluate_tracks(str(tmp_path / "clip_selected_data.csv"), str(tmp_path / name), df=df, settings=settings, fps=30.0)
    files = sorted(os.listdir(tmp_path / "host"))
    assert files == sorted(os.listdir(tmp_path / "device"))
    pngs = [f for f in files if f.endswith(".png")]
    assert len(pngs) == 11                                                    # three track figures, eight violin figures
    for f in files:
        if f not in pngs:
            assert (tmp_path / "host" / f).read_bytes() == (tmp_path / "device" / f).read_bytes()
    for f in pngs:
        want, wc = png_tools.read_png(str(tmp_path / "host" / f))
        got, gc = png_tools.read_png(str(tmp_path / "device" / f))
        assert wc[b"IHDR"] == gc[b"IHDR"] and wc[b"pHYs"] == gc[b"pHYs"] and wc["order"] == gc["order"], f
        assert np.array_equal(got, want), "{}: {} pixels differ".format(f, (got != want).any(axis=2).sum())
        assert (want != 255).any()
