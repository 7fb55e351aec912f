"""The track figures without a GPU: the C ABI's new entry points and their argument checks, the colour table, the
rendering model's two forms, the PNG writer, ticks and view, the lettering, and the wiring in ``evaluate_tracks``."""
import ctypes
import os
import re

import numpy as np
import pytest

import plot_model as pm
import png_tools
from conftest import ROOT

NEW = ("ysmr_plot_colormap", "ysmr_plot_extent", "ysmr_plot_workspace_bytes", "ysmr_plot_tracks", "ysmr_plot_angle_histogram",
       "ysmr_plot_wedges")


@pytest.fixture(scope="module")
def lib():
    from ysmr_amd import _lib
    return _lib.lib()


def test_plot_entry_points_are_declared_exported_and_bound(lib):
    from ysmr_amd import _lib
    header = open(os.path.join(ROOT, "include", "ysmr_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name + " is not declared in include/ysmr_hip.h"
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"}\s*ysmr_plot_view;", header)
    assert int(re.search(r"#define YSMR_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 15
    assert lib.ysmr_plot_workspace_bytes.restype is ctypes.c_size_t and lib.ysmr_plot_tracks.restype is ctypes.c_int
    # the struct as the header lays it out: four doubles, fifteen ints, two arrays of 32
    assert ctypes.sizeof(_lib.PlotView) == 4 * 8 + 15 * 4 + 2 * 32 * 4 + 4
    assert _lib.PlotView.mode.offset == 32 and _lib.PlotView.grid_cols.offset == 92
    assert "plots.hip" in open(os.path.join(ROOT, "ysmr_amd", "csrc", "Makefile")).read()


def test_colormap_is_viridis_r(lib):
    out = (ctypes.c_uint8 * 768)()
    assert lib.ysmr_plot_colormap(out) == 0
    got = np.frombuffer(out, np.uint8).reshape(256, 3)
    assert np.array_equal(got, pm.lut())
    assert got[0].tolist() == [253, 231, 36] and got[255].tolist() == [68, 1, 84]
    try:
        from matplotlib import cm
    except ImportError:
        return
    assert np.array_equal(got, np.array([cm.viridis_r(k, bytes=True)[:3] for k in range(256)], np.uint8))


def _view(**kw):
    v = pm.to_struct(pm.make_view(0, 96, 64, (10, 6, 70, 50), 0.0, 0.0, 1.0))
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def test_plot_entry_points_reject_bad_arguments(lib):
    from ysmr_amd import _lib
    some = ctypes.c_void_p(4096)          # never dereferenced: every call below fails its argument checks
    ARG = _lib.YSMR_ERR_ARG
    assert lib.ysmr_plot_colormap(None) == ARG
    # extent
    assert lib.ysmr_plot_extent(None, 4, some, some, some, 0, 1.0, None) == ARG and b"NULL" in lib.ysmr_last_error()
    assert lib.ysmr_plot_extent(None, 4, some, None, some, 0, 1.0, some) == ARG
    assert lib.ysmr_plot_extent(None, 4, None, some, some, 1, 1.0, some) == ARG
    assert lib.ysmr_plot_extent(None, 4, some, some, some, 2, 1.0, some) == ARG and b"mode" in lib.ysmr_last_error()
    assert lib.ysmr_plot_extent(None, 4, some, some, some, 0, 0.0, some) == ARG and b"px" in lib.ysmr_last_error()
    assert lib.ysmr_plot_extent(None, -1, some, some, some, 0, 1.0, some) == ARG
    # tracks
    def tracks(view, n=4, ids=some, x=some, y=some, nt=2, dist=some, stride=1, ws=some, nbytes=1 << 30, rgb=some):
        return lib.ysmr_plot_tracks(None, n, ids, x, y, nt, dist, stride, ctypes.byref(view) if view is not None else None, ws,
                                    nbytes, rgb)
    assert tracks(None) == ARG
    for bad in (dict(ids=None), dict(x=None), dict(y=None), dict(dist=None), dict(ws=None), dict(rgb=None)):
        assert tracks(_view(), **bad) == ARG and b"NULL" in lib.ysmr_last_error(), bad
    for bad in (dict(ax_x=-1), dict(ax_y=-1), dict(ax_w=0), dict(ax_h=0), dict(ax_x=27), dict(ax_y=15), dict(ax_w=87)):
        assert tracks(_view(**bad)) == ARG and b"axes rectangle" in lib.ysmr_last_error(), bad
    assert tracks(_view(bar_x=90, bar_y=6, bar_w=7, bar_h=50)) == ARG and b"colour bar" in lib.ysmr_last_error()
    for bad in (dict(mode=2), dict(px=0.0), dict(units_per_pixel=0.0), dict(u0=float("nan")), dict(r2_dot=-1), dict(r2_start=4097),
                dict(n_grid_cols=33), dict(width=0)):
        assert tracks(_view(**bad)) == ARG, bad
    assert tracks(_view(), stride=0) == ARG
    assert tracks(_view(), nbytes=16) == 3 and b"workspace" in lib.ysmr_last_error()           # YSMR_ERR_CAPACITY
    assert lib.ysmr_plot_workspace_bytes(-1, 0, 4, 4) == 0 and lib.ysmr_plot_workspace_bytes(4, 2, 96, 64) >= 96 * 64 * 4
    assert lib.ysmr_plot_workspace_bytes(4, 0, 0, 0) > 0
    # histogram
    def hist(n=4, ids=some, x=some, y=some, mv=some, lag=1, bins=36, edges=some, ws=some, nbytes=1 << 30, counts=some, points=some):
        return lib.ysmr_plot_angle_histogram(None, n, ids, x, y, mv, lag, bins, edges, ws, nbytes, counts, points)
    for bad in (dict(bins=0), dict(bins=1025)):
        assert hist(**bad) == ARG and b"n_bins" in lib.ysmr_last_error(), bad
    for bad in (dict(ids=None), dict(x=None), dict(y=None), dict(mv=None), dict(edges=None), dict(ws=None), dict(counts=None),
                dict(points=None)):
        assert hist(**bad) == ARG and b"NULL" in lib.ysmr_last_error(), bad
    assert hist(lag=0) == ARG and hist(n=-1) == ARG
    assert hist(nbytes=16) == 3
    # wedges
    def wedges(W=64, H=64, cx=32, cy=32, bins=8, dirs=some, r2=some, ring=100, rgb=some):
        return lib.ysmr_plot_wedges(None, W, H, cx, cy, bins, dirs, r2, ring, rgb)
    for bad in (dict(bins=2), dict(bins=1025)):
        assert wedges(**bad) == ARG and b"n_bins" in lib.ysmr_last_error(), bad
    for bad in (dict(dirs=None), dict(r2=None), dict(rgb=None)):
        assert wedges(**bad) == ARG and b"NULL" in lib.ysmr_last_error(), bad
    for bad in (dict(W=0), dict(H=0), dict(ring=-1), dict(cx=1 << 21)):
        assert wedges(**bad) == ARG, bad


# ---- the model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_sequential_painter_equals_largest_key_wins(seed, mode):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 30, 9)
    ids = np.repeat(np.arange(9) * 3 + 1, lengths)
    n = len(ids)
    x, y = rng.uniform(-8, 90, n), rng.uniform(-8, 60, n)
    x[rng.integers(0, n)] = np.nan
    dist = rng.uniform(0, 20, 9)
    dist[4] = dist[2]
    view = pm.make_view(mode, 96, 64, (10, 6, 70, 50), -3.0 if mode == 0 else -40.0, 2.0 if mode == 0 else -30.0, 1.25,
                        px=1.3, r2_dot=int(rng.choice([0, 1, 5])), r2_start=4, grid_cols=[20, 47], grid_rows=[30], bar=(85, 6, 5, 50))
    a, b = pm.key_canvas_sequential(ids, x, y, dist, view), pm.key_canvas_max(ids, x, y, dist, view)
    assert np.array_equal(a, b) and len(np.unique(a)) > 4
    assert np.array_equal(pm.paint_tracks(ids, x, y, dist, view, sequential=True), pm.paint_tracks(ids, x, y, dist, view))


def test_model_colour_values_and_ranks():
    c, idx, rank = pm.colour_values([3.0, 1.0, 5.0, 1.0, 5.0])
    assert c.tolist() == [0.5, 0.0, 1.0, 0.0, 1.0] and idx.tolist() == [128, 0, 255, 0, 255]
    assert rank.tolist() == [2, 3, 0, 4, 1]                   # longest first; among equals the earlier track first
    for flat in ([2.0, 2.0, 2.0], [1.0, np.nan], [0.0, np.inf], [7.0]):
        c, idx, rank = pm.colour_values(flat)
        assert not c.any() and not idx.any() and rank.tolist() == list(range(len(flat)))


# ---- PNG -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 5, 131])
def test_png_round_trip(tmp_path, width):
    from ysmr_amd.plot_functions import write_png
    rgb = np.random.default_rng(width).integers(0, 256, (7, width, 3), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    write_png(path, rgb, dpi=300)
    back, chunks = png_tools.read_png(path)
    assert np.array_equal(back, rgb)
    assert chunks["order"] == [b"IHDR", b"pHYs", b"IDAT", b"IEND"]
    assert chunks[b"pHYs"] == (11811).to_bytes(4, "big") * 2 + b"\x01"
    with pytest.raises(ValueError):
        write_png(path, rgb[:, :, :2])


# ---- ticks and view --------------------------------------------------------------------------------------------------

def test_ticks_follow_1_2_5():
    from ysmr_amd.plot_functions import nice_step, ticks_125
    assert [nice_step(s) for s in (8.0, 9.0, 17.0, 41.0, 0.8, 1234.0)] == [1.0, 2.0, 5.0, 10.0, 0.1, 200.0]
    assert nice_step(0.0) == 1.0 and nice_step(float("nan")) == 1.0
    assert ticks_125(-0.25, 0.35, 0.1).tolist() == [-0.2, -0.1, 0.0, 0.1, 0.2, 0.3]
    assert ticks_125(3.0, 2.0, 1.0).tolist() == [] and len(ticks_125(0.0, 1000.0, 1.0)) == 32


@pytest.mark.parametrize("extent", [(5.0, 5.0, 7.0, 7.0), (0.0, 100.0, 5.0, 5.0), (np.inf, -np.inf, np.inf, -np.inf),
                                    (-3.0, 40.0, 2.0, 90.0)])
def test_view_for_degenerate_extents(extent):
    from ysmr_amd.plot_functions import track_view
    view, cols, rows = track_view(extent, 0, 1.4, dpi=300)
    assert (view.width, view.height) == (3507, 2480) and view.r2_dot == 1 and view.r2_start == 4
    assert view.units_per_pixel > 0 and np.isfinite([view.u0, view.v0, view.units_per_pixel]).all()
    assert 0 <= view.ax_x and view.ax_x + view.ax_w < view.bar_x - 1 and view.bar_x + view.bar_w <= view.width
    assert 0 <= view.ax_y and view.ax_y + view.ax_h <= view.height
    lo_u, hi_u, lo_v, hi_v = extent if np.isfinite(extent).all() else (0.0, 1.0, 0.0, 1.0)
    # the extent lies inside the view with its margin, centred
    right, top = view.u0 + view.units_per_pixel * view.ax_w, view.v0 + view.units_per_pixel * view.ax_h
    assert view.u0 < lo_u and hi_u < right and view.v0 < lo_v and hi_v < top
    assert abs((view.u0 + right) - (lo_u + hi_u)) < 1e-9 * max(1.0, abs(right)) and abs((view.v0 + top) - (lo_v + hi_v)) < 1e-9 * max(1.0, abs(top))
    assert 2 <= len(cols) <= 32 and 1 <= len(rows) <= 32 and view.n_grid_cols == len(cols) and view.n_grid_rows == len(rows)
    assert all(view.ax_x <= c < view.ax_x + view.ax_w for _, c in cols) and all(view.ax_y <= r < view.ax_y + view.ax_h for _, r in rows)
    steps = np.diff([t for t, _ in cols])
    assert np.allclose(steps, steps[0]) and float("{:.0e}".format(steps[0])[0]) in (1.0, 2.0, 5.0)


def test_view_scales_the_dots_with_dpi():
    from ysmr_amd.plot_functions import track_view
    view, _, _ = track_view((0.0, 1.0, 0.0, 1.0), 1, 1.0, dpi=600)
    assert (view.width, view.height, view.r2_dot, view.r2_start, view.mode) == (7015, 4960, 4, 16, 1)


# ---- lettering -------------------------------------------------------------------------------------------------------

def test_font_stamping_and_clipping():
    from ysmr_amd.plot_functions import stamp_text, text_bitmap, text_size
    one = text_bitmap("1")
    assert ["".join("#" if v else "." for v in r) for r in one] == ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."]
    assert text_bitmap("µm").shape == (7, 11) and text_bitmap("µ").any() and not text_bitmap(" ").any()
    assert np.array_equal(text_bitmap("☃"), text_bitmap("?"))                       # not in the font
    assert text_bitmap("ab", 3).shape == (21, 33) == text_size("ab", 3)[::-1]
    assert np.array_equal(text_bitmap("ab", 3)[::3, ::3], text_bitmap("ab"))
    assert len({text_bitmap(chr(c)).tobytes() for c in range(33, 127)}) == 94           # all different
    canvas = np.full((20, 30, 3), 255, np.uint8)
    stamp_text(canvas, 2, 3, "A1", colour=(9, 8, 7))
    on = (canvas == (9, 8, 7)).all(axis=2)
    assert np.array_equal(on[3:10, 2:13], text_bitmap("A1")) and on.sum() == text_bitmap("A1").sum()
    # clipped at every edge: what is inside is stamped, nothing else is touched, nothing raises
    for x, y in ((-3, -2), (26, 16), (-3, 16), (26, -2), (-40, 5), (5, 40)):
        canvas = np.full((20, 30, 3), 255, np.uint8)
        stamp_text(canvas, x, y, "W8", scale=2)
        big = np.zeros((120, 150), bool)
        bm = text_bitmap("W8", 2)
        big[50 + y:50 + y + bm.shape[0], 60 + x:60 + x + bm.shape[1]] = bm
        assert np.array_equal((canvas == 0).all(axis=2), big[50:70, 60:90])
    canvas = np.full((20, 30, 3), 255, np.uint8)
    stamp_text(canvas, 15, 0, "ab", anchor="centre")
    stamp_text(canvas, 30, 10, "ab", anchor="right")
    on = (canvas == 0).all(axis=2)
    assert np.array_equal(on[0:7, 10:21], text_bitmap("ab")) and np.array_equal(on[10:17, 19:30], text_bitmap("ab"))


# ---- the wiring ------------------------------------------------------------------------------------------------------

def _table(n_tracks=4, rows=12):
    import pandas as pd
    rng = np.random.default_rng(5)
    ids = np.repeat(np.arange(n_tracks, dtype=np.uint32) + 3, rows)
    t = np.tile(np.arange(rows, dtype=np.uint32), n_tracks)
    return pd.DataFrame({"TRACK_ID": ids, "POSITION_T": t, "POSITION_X": rng.uniform(0, 50, len(ids)),
                         "POSITION_Y": rng.uniform(0, 50, len(ids)), "WIDTH": 4.0, "HEIGHT": 2.0, "DEGREES_ANGLE": -10.0})


def _stub_device(monkeypatch, calls, fail=None):
    from ysmr_amd import evaluate, plot_functions as pf

    def columns(df, params, device="cuda:0"):
        n = len(df)
        rows = {"WIDTH": np.full(n, 2.8), "HEIGHT": np.full(n, 1.4), "angle_diff": np.zeros(n, np.int32),
                "moving": np.ones(n, np.int8), "turn_points": np.zeros(n, np.int8), "tp_of_tracks": np.zeros(n),
                "travelled_dist": np.full(n, 0.5), "motility_phenotype": np.full(n, 2, np.int8)}
        ids = df["TRACK_ID"].to_numpy()
        stats = np.zeros((len(np.unique(ids)), 12))
        stats[:, 1] = np.arange(len(stats)) + 6.0
        stats[:, 3] = 0.4
        stats[:, 9] = 2
        stats[:, 10] = np.unique(ids)
        return rows, stats

    def tracks(ids, x, y, dist, view, dev):
        if fail == "tracks":
            raise RuntimeError("no canvas today")
        calls.append(("tracks", view.mode, np.asarray(dist).tolist(), view.px))
        return np.full((view.height, view.width, 3), 255, np.uint8)

    def histogram(ids, x, y, moving, lag, edges, dev):
        calls.append(("histogram", lag, len(edges) - 1))
        return np.arange(len(edges) - 1, dtype=np.int64), 0 if fail == "no points" else 40

    def wedges(W, H, cx, cy, dirs, r2, ring_r2, dev):
        calls.append(("wedges", W, H, len(r2)))
        return np.full((H, W, 3), 255, np.uint8)

    monkeypatch.setattr(evaluate, "evaluate_columns", columns)
    monkeypatch.setattr(pf, "_upload", lambda df, dev, moving=False: (None,) * (4 if moving else 3))
    monkeypatch.setattr(pf, "device_extent", lambda ids, x, y, mode, px, dev: np.array([0.0, 30.0, 0.0, 20.0]))
    monkeypatch.setattr(pf, "device_tracks", tracks)
    monkeypatch.setattr(pf, "device_angle_histogram", histogram)
    monkeypatch.setattr(pf, "device_wedges", wedges)


def _settings(**kw):
    from ysmr_amd.helper_file import default_settings
    return default_settings(**dict({"user input": False, "select files": False, "log to file": False}, **kw))


OFF = {"save large plots": False, "save rose plot": False, "save angle distribution plot / bins": 0}


def _run(tmp_path, name, settings):
    from ysmr_amd.evaluate import evaluate_tracks
    out = tmp_path / name
    out.mkdir()
    res = evaluate_tracks(str(tmp_path / "210102030405_clip_selected_data.csv"), str(out), df=_table(), settings=settings, fps=30.0)
    return res, {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}


def test_evaluate_tracks_writes_the_figures_its_settings_ask_for(tmp_path, monkeypatch, caplog):
    import logging
    from ysmr_amd import plot_functions as pf
    caplog.set_level(logging.INFO, logger="ysmr")
    calls = []
    _stub_device(monkeypatch, calls)
    (df_off, stats_off), files_off = _run(tmp_path, "off", _settings(**OFF))
    prefix = "210102030405_clip_selected_data_"
    assert sorted(files_off) == [prefix + "analysed.csv", prefix + "statistics.csv"] and calls == []
    assert "save large plots" not in caplog.text and "save time violin plot" in caplog.text       # only what is still skipped
    # the defaults: all three
    (df_on, stats_on), files_on = _run(tmp_path, "on", _settings())
    assert sorted(files_on) == [prefix + n for n in ("Bac_Run_Overview.png", "analysed.csv", "angle_histogram.png", "rose_graph.png",
                                                     "statistics.csv")]
    assert [c[0] for c in calls] == ["histogram", "wedges", "tracks", "tracks"]
    assert calls[0] == ("histogram", 10, 36) and calls[1] == ("wedges", 3507, 2480, 36)
    assert calls[2] == ("tracks", 0, [6.0, 7.0, 8.0, 9.0], 1.41888781) and calls[3] == ("tracks", 1, [6.0, 7.0, 8.0, 9.0], 1.41888781)
    assert df_on.equals(df_off) and stats_on.equals(stats_off)
    assert all(files_on[k] == files_off[k] for k in files_off)
    rgb, chunks = png_tools.read_png(str(tmp_path / "on" / (prefix + "Bac_Run_Overview.png")))
    assert rgb.shape == (2480, 3507, 3) and chunks[b"pHYs"][:4] == (11811).to_bytes(4, "big")
    view, _, _ = pf.track_view([0.0, 30.0, 0.0, 20.0], 0, 1.41888781)
    assert (rgb[view.ax_y:view.ax_y + view.ax_h, view.ax_x:view.ax_x + view.ax_w] == 255).all()    # lettering stays outside the axes
    title = rgb[:view.ax_y - 1]
    assert (title == 0).all(axis=2).any()                                                          # "02. 01. '21,  clip"
    # one key at a time
    for key, value, name in (("save large plots", True, "Bac_Run_Overview.png"), ("save rose plot", True, "rose_graph.png"),
                             ("save angle distribution plot / bins", 7, "angle_histogram.png")):
        calls.clear()
        _, files = _run(tmp_path, name[:4], _settings(**dict(OFF, **{key: value})))
        assert sorted(files) == sorted([prefix + name, prefix + "analysed.csv", prefix + "statistics.csv"])
    assert calls == [("histogram", 10, 7), ("wedges", 3507, 2480, 7)]


def test_a_failing_figure_leaves_the_results_intact(tmp_path, monkeypatch, caplog):
    calls = []
    _stub_device(monkeypatch, calls)
    (df_ref, stats_ref), files_ref = _run(tmp_path, "ref", _settings(**OFF))
    _stub_device(monkeypatch, calls, fail="tracks")
    (df, stats), files = _run(tmp_path, "fail", _settings())
    prefix = "210102030405_clip_selected_data_"
    assert sorted(files) == [prefix + "analysed.csv", prefix + "angle_histogram.png", prefix + "statistics.csv"]
    assert caplog.text.count("no canvas today") == 2 and "Bac_Run_Overview.png failed" in caplog.text
    assert df.equals(df_ref) and stats.equals(stats_ref) and all(files[k] == files_ref[k] for k in files_ref)
    # no motile tracks: upstream's warning, no file
    _stub_device(monkeypatch, calls, fail="no points")
    _, files = _run(tmp_path, "none", _settings(**dict(OFF, **{"save angle distribution plot / bins": 36})))
    assert sorted(files) == [prefix + "analysed.csv", prefix + "statistics.csv"]
    assert "Cannot create angle distribution plot as there are no motile tracks." in caplog.text


def test_plot_title_and_package_surface():
    import ysmr_amd
    from ysmr_amd import plot_functions as pf
    from ysmr_amd.evaluate import plot_title
    assert plot_title("210102030405_clip_selected_data") == "02. 01. '21,  clip"
    assert plot_title("my_clip_selected_data") == "my clip" and plot_title("999999999999_x") == "999999999999 x"
    assert ysmr_amd.large_xy_plot is pf.large_xy_plot and ysmr_amd.rose_graph is pf.rose_graph
    assert ysmr_amd.angle_distribution_plot is pf.angle_distribution_plot
    assert pf.__all__ == ["angle_distribution_plot", "large_xy_plot", "rose_graph"]
