"""``ysmr_png_deflate_dynamic`` on the device (csrc/png.hip, csrc/png_codes.h) against tests/png_dynamic_model.py byte for byte
and against zlib, its argument checks, the files ``write_png_device(..., dynamic=True)`` writes, and every figure of
``evaluate_tracks`` with 'hip png on device' set to 'dynamic'."""
import os
import zlib

import numpy as np
import pytest

import png_deflate_model as pm
import png_dynamic_model as dm
import png_tools

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _idat(path):
    """The body of the file's IDAT chunk (png_tools.read_png has checked the CRCs and that the chunks end the file)."""
    raw = open(path, "rb").read()
    at = 8
    while raw[at + 4:at + 8] != b"IDAT":
        at += 12 + int.from_bytes(raw[at:at + 4], "big")
    return raw[at + 8:at + 8 + int.from_bytes(raw[at:at + 4], "big")]


def _deflate(rgb, dynamic=True):
    import torch
    from ysmr_amd import plot_functions as pf
    return pf.device_deflate(torch.from_numpy(np.array(rgb)).to(DEV), dynamic=dynamic)


@pytest.mark.parametrize("case_id", dm.CASE_IDS)
def test_stream_is_the_models_byte_for_byte(case_id):
    from ysmr_amd import _lib
    rgb, want = dm.case(case_id)
    got = _deflate(rgb)
    h, w = rgb.shape[:2]
    assert len(got) <= _lib.lib().ysmr_png_dynamic_stream_bytes_max(w, h)
    assert zlib.decompress(got) == pm.scanlines(rgb).tobytes()
    assert len(got) == len(want), "{} bytes, the model has {}".format(len(got), len(want))
    diff = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert not len(diff), "{} bytes differ, the first at {}".format(len(diff), diff[0])


@pytest.mark.parametrize("case_id", dm.RANDOM_LITERAL_IDS)
def test_random_literals_fit_the_documented_bound(case_id):
    from ysmr_amd import _lib
    rgb = dm.canvas(case_id)
    h, w = rgb.shape[:2]
    got = _deflate(rgb)
    assert len(got) <= dm.stream_bytes_bound(w, h) <= _lib.lib().ysmr_png_dynamic_stream_bytes_max(w, h)
    assert zlib.decompress(got) == pm.scanlines(rgb).tobytes()


def test_full_size_canvas_twice():
    """3507 x 2480 with 3000 discs: two runs give identical bytes, they inflate to the scanline bytes and are fewer than the
    fixed stream's."""
    import torch
    from ysmr_amd import plot_functions as pf
    rgb = pm.discs_canvas()
    dev = torch.from_numpy(rgb).to(DEV)
    first, second = pf.device_deflate(dev, dynamic=True), pf.device_deflate(dev, dynamic=True)
    assert first == second
    raw = pm.scanlines(rgb).tobytes()
    d = zlib.decompressobj()
    assert d.decompress(first) == raw and d.eof and d.unused_data == b""
    assert first[:2] == b"\x78\x01" and first[2] & 7 == 0b101
    assert int.from_bytes(first[-4:], "big") == zlib.adler32(raw) & 0xFFFFFFFF
    fixed = pf.device_deflate(dev)
    print("discs 3507 x 2480: dynamic {} B, fixed {} B".format(len(first), len(fixed)))
    assert len(first) < len(fixed)


def test_bad_arguments_are_refused():
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    w, h = 85, 2
    rgb = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.ysmr_png_dynamic_workspace_bytes(w, h) + 8, dtype=torch.uint8, device=DEV)
    out = torch.empty(L.ysmr_png_dynamic_stream_bytes_max(w, h) + 8, dtype=torch.uint8, device=DEV)
    n = torch.zeros(2, dtype=torch.int64, device=DEV)
    good = dict(rgb=rgb.data_ptr(), w=w, h=h, ws=ws.data_ptr(), ws_bytes=ws.numel() - 8, out=out.data_ptr(), out_bytes=out.numel() - 8, n=n.data_ptr())

    def call(**change):
        a = dict(good, **change)
        return L.ysmr_png_deflate_dynamic(_lib.stream_ptr(DEV), a["rgb"], a["w"], a["h"], a["ws"], a["ws_bytes"], a["out"], a["out_bytes"], a["n"])

    for change in (dict(ws_bytes=good["ws_bytes"] - 1), dict(out_bytes=good["out_bytes"] - 1), dict(rgb=None), dict(ws=None), dict(out=None),
                   dict(n=None), dict(ws=good["ws"] + 4), dict(out=good["out"] + 2), dict(n=good["n"] + 4), dict(w=0), dict(h=0),
                   dict(w=16385), dict(h=16385), dict(w=-3)):
        assert call(**change) == _lib.YSMR_ERR_ARG, change
    assert call() == _lib.YSMR_OK
    assert zlib.decompress(out[:int(n[0].item())].cpu().numpy().tobytes()) == bytes(h * (1 + 3 * w))


def test_write_png_device_lays_the_file_out_as_write_png(tmp_path):
    import torch
    from ysmr_amd import plot_functions as pf
    rgb, _ = pm.case("periods-341x67")
    pf.write_png(str(tmp_path / "host.png"), rgb, 150)
    pf.write_png_device(str(tmp_path / "device.png"), torch.from_numpy(np.array(rgb)).to(DEV), 150, dynamic=True)
    host, hc = png_tools.read_png(str(tmp_path / "host.png"))
    dev, dc = png_tools.read_png(str(tmp_path / "device.png"))
    assert np.array_equal(host, rgb) and np.array_equal(dev, rgb)
    assert hc["order"] == dc["order"] == [b"IHDR", b"pHYs", b"IDAT", b"IEND"]
    assert hc[b"IHDR"] == dc[b"IHDR"] and hc[b"pHYs"] == dc[b"pHYs"]
    assert _idat(str(tmp_path / "device.png")) == dm.case("periods-341x67")[1]
    assert zlib.decompress(_idat(str(tmp_path / "device.png"))) == zlib.decompress(_idat(str(tmp_path / "host.png"))) == pm.scanlines(rgb).tobytes()


def test_evaluate_tracks_writes_the_same_smaller_figures_with_dynamic(tmp_path):
    from select_tables import make_table, select_settings
    from ysmr_amd import evaluate_tracks
    df = make_table(5, n_tracks=25, max_len=500)
    size = df.groupby("TRACK_ID")["TRACK_ID"].transform("size")
    df = df[size >= 32].reset_index(drop=True)
    host = select_settings(**{"store generated statistical .csv file": True, "store final analysed .csv file": True,
                              "hip violin plots": True})
    assert "hip png on device" not in host
    runs = (("host", host), ("fixed", dict(host, **{"hip png on device": True})), ("dynamic", dict(host, **{"hip png on device": "Dynamic"})))
    for name, settings in runs:
        os.makedirs(tmp_path / name)
        evaluate_tracks(str(tmp_path / "clip_selected_data.csv"), str(tmp_path / name), df=df, settings=settings, fps=30.0)
    files = sorted(os.listdir(tmp_path / "host"))
    assert files == sorted(os.listdir(tmp_path / "dynamic")) == sorted(os.listdir(tmp_path / "fixed"))
    pngs = [f for f in files if f.endswith(".png")]
    assert len(pngs) == 11                                                    # three track figures, eight violin figures
    for f in pngs:
        want, wc = png_tools.read_png(str(tmp_path / "host" / f))
        got, gc = png_tools.read_png(str(tmp_path / "dynamic" / f))
        assert wc[b"IHDR"] == gc[b"IHDR"] and wc[b"pHYs"] == gc[b"pHYs"] and wc["order"] == gc["order"], f
        assert np.array_equal(got, want), "{}: {} pixels differ".format(f, (got != want).any(axis=2).sum())
        assert (want != 255).any()
        assert _idat(str(tmp_path / "dynamic" / f))[2] & 7 == 0b101, f                                # it is the dynamic stream
        sizes = [os.path.getsize(tmp_path / name / f) for name in ("host", "fixed", "dynamic")]
        print("{}: host {} B, fixed {} B, dynamic {} B".format(f, *sizes))
        assert sizes[2] <= sizes[1], f


def test_true_still_gives_the_fixed_stream():
    """A guard: the old path was not touched."""
    rgb, want = pm.case("periods-341x67")
    assert _deflate(rgb, dynamic=False) == want
