"""GPU: the violin kernels (csrc/violin.hip) against the NumPy model of their rules (violin_model.py) -- categories,
counts and order statistics bit for bit, moments and densities at the bounds written below, profile and painter byte
for byte -- and the eight figures end to end through evaluate_tracks."""
import os

import numpy as np
import pytest

import png_tools
import violin_model as vm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXACT = ("members", "values", "vmin", "vmax", "q25", "q50", "q75", "whisker_lo", "whisker_hi")


def _stats(cut, value, lo, hi):
    from ysmr_amd.plot_functions import device_violin_stats
    return device_violin_stats(cut, value, lo, hi, DEV)


def _assert_summaries(got, want):
    """Counts and order statistics bit for bit; mean and h within 1e-13 relative (a two-pass fixed-order sum is good to a
    few log2 n ulps: this is about 50 x that and far below a wrong ddof, 1.2e-4 at n = 4096)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    for name in EXACT:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])
    for name in ("mean", "h"):
        err = np.abs(got[name] - want[name])
        print(name, "worst relative error", float(np.max(err / np.maximum(np.abs(want[name]), 1e-300))))
        assert np.all(err <= 1e-13 * np.abs(want[name])), (name, got[name], want[name])


def _assert_densities(got, want):
    """Every grid point within 1e-12 x the model's grid peak (the formula's bound is about (8 + log2 n) 2^-53 of the peak
    with an exp good to an ulp or so)."""
    assert got.shape == want.shape
    for v in range(len(want)):
        peak = want[v].max()
        worst = float(np.abs(got[v] - want[v]).max())
        print("violin", v, "worst density error / peak", worst / peak if peak > 0 else worst)
        assert worst <= 1e-12 * peak, (v, worst, peak)


# ---- categories and counts -------------------------------------------------------------------------------------------

def _category_table():
    rng = np.random.default_rng(3)
    cut = np.concatenate([[0.0, 20.0, 40.0, 100.01, 100.0, 19.999999999999996, -1e-300, np.nan, np.nan, np.inf, -np.inf],
                          rng.uniform(-5, 105, 300), [1.0, 2.0, 0.0, 0.001, 1.001, 2.0009999999999994]])
    value = np.round(rng.gamma(2.0, 3.0, len(cut)), 2)
    value[[1, 7, 30, 31]] = np.nan
    value[[2, 40]] = np.inf
    value[41] = -np.inf
    cut[(cut >= 60) & (cut < 80)] = 59.5                 # an empty category
    return cut, value


SPLITS = {"default": ([0.0, 20.0, 40.0, 60.0, 80.0], [20.0, 40.0, 60.0, 80.0, 100.01]),
          "overlapping": ([0.0, 10.0, 5.0, 50.0, 90.0, 30.0], [30.0, 20.0, 15.0, 40.0, np.inf, 95.0]),
          "phenotype": ([0.0, 1.0, 2.0], [0.001, 1.001, 2.001]),
          "none": ([], [])}


@pytest.mark.parametrize("split", sorted(SPLITS))
def test_categories_and_counts_are_bit_exact(split):
    cut, value = _category_table()
    lo, hi = SPLITS[split]
    want, want_d = vm.stats(cut, value, lo, hi)
    got, got_d = _stats(cut, value, lo, hi)
    _assert_summaries(got, want)
    _assert_densities(got_d, want_d)
    assert want["members"][0] == len(cut) and want["values"][0] == len(cut) - 7
    if split == "default":
        assert want["members"][4] == 0 and (want["members"][1:] > 0).sum() == 4
        assert want["members"][1:].sum() < len(cut) - 2              # NaN and out-of-range cuts are in no category
    if split == "overlapping":
        cat = vm.categories(cut, lo, hi)
        assert want["members"][4] == 0 and (cat[(cut >= 10) & (cut < 15)] == 3).all() and (cat[(cut >= 90) & (cut < 95)] == 6).all()
    if split == "phenotype":
        assert want["members"][1:].tolist() == [2, 1, 2]              # 0.001 and 1.001 are outside: the upper ends are open
    again, again_d = _stats(cut, value, lo, hi)
    assert again.tobytes() == got.tobytes() and again_d.tobytes() == got_d.tobytes()


# ---- summaries and densities -----------------------------------------------------------------------------------------

SIZES = (0, 1, 2, 3, 17, 257, 4099)      # one wave, one 256-lane workgroup, and (two entries per track) nine 2048-key sort tiles


@pytest.fixture(scope="module")
def sized():
    """One table whose categories hold 0, 1, 2, 3, 17, 257 and 4099 values, ties, all-equal values and a whisker on the
    outlier boundary: (cut, value, lo, hi, model summaries, model densities, device summaries, device densities)."""
    rng = np.random.default_rng(17)
    groups = [rng.gamma(2.0, 3.0, n) for n in SIZES]
    groups[4] = np.round(rng.uniform(0, 3, 17), 1)                                   # ties
    groups.append(np.full(5, 3.25))                                                 # h == 0
    groups.append(np.array([-2.0, 1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 6.0, 9.0]))    # fences at -2 and 6, both values
    groups.append(np.concatenate([rng.normal(50.0, 1e-3, 1000)]))                   # tightly clustered
    cut = np.concatenate([np.full(len(g), k + 0.5) for k, g in enumerate(groups)])
    value = np.concatenate(groups)
    order = rng.permutation(len(cut))
    cut, value = cut[order], value[order]
    lo, hi = np.arange(len(groups), dtype=np.float64), np.arange(len(groups), dtype=np.float64) + 1.0
    want, want_d = vm.stats(cut, value, lo, hi)
    got, got_d = _stats(cut, value, lo, hi)
    return cut, value, lo, hi, want, want_d, got, got_d


def test_summaries_match_the_model(sized):
    cut, value, lo, hi, want, want_d, got, got_d = sized
    assert want["values"][1:].tolist() == list(SIZES) + [5, 10, 1000]
    _assert_summaries(got, want)
    assert want["h"][8] == 0.0 and want["h"][2] == 0.0 and want["h"][3] > 0
    assert (want["whisker_lo"][9], want["whisker_hi"][9], want["vmax"][9]) == (-2.0, 6.0, 9.0)
    assert got[1].tobytes() == np.zeros((), vm.SUMMARY_DTYPE).tobytes()             # a violin without a value does not exist


def test_densities_match_the_model(sized):
    cut, value, lo, hi, want, want_d, got, got_d = sized
    _assert_densities(got_d, want_d)
    for v in (1, 2, 8):                                                             # no value, one value, h == 0: no density
        assert not got_d[v].any()
    assert (want_d[[0, 3, 4, 5, 6, 7, 9, 10]].max(axis=1) > 0).all()
    again, again_d = _stats(cut, value, lo, hi)
    assert again.tobytes() == got.tobytes() and again_d.tobytes() == got_d.tobytes()


# ---- profile and painter ---------------------------------------------------------------------------------------------

def _summary(values, vmin, vmax, h, members=None):
    s = np.zeros((), vm.SUMMARY_DTYPE)
    s["members"], s["values"] = values if members is None else members, values
    if values:
        span = vmax - vmin
        s["vmin"], s["vmax"], s["h"] = vmin, vmax, h
        s["q25"], s["q50"], s["q75"] = vmin + 0.3 * span, vmin + 0.45 * span, vmin + 0.7 * span
        s["whisker_lo"], s["whisker_hi"], s["mean"] = vmin + 0.1 * span, vmin + 0.95 * span, vmin + 0.5 * span
    return s


def _bell(centre, width):
    j = np.arange(vm.GRID, dtype=np.float64)
    return np.exp(-0.5 * ((j - centre) / width) ** 2) / 7.0


def _six():
    """96 x 64, six slots of 13 pixels, y from 0 to 25."""
    sums = np.array([_summary(100, 2.0, 20.0, 0.7),        # the full count: touches both edges of its slot at its peak
                     _summary(1, 12.3, 12.3, 0.0),         # one value: a line
                     _summary(70, -5.0, 10.0, 0.5),        # partly below the axes
                     _summary(90, 30.0, 40.0, 0.5),        # wholly above
                     _summary(60, 1.0, 24.0, 0.1),         # a peak of one grid point
                     _summary(2, 3.0, 22.0, 0.4)])         # two values beside a hundred: half width 0
    spike = np.zeros(vm.GRID)
    spike[50] = 1.0
    dens = np.stack([_bell(40, 12), np.zeros(vm.GRID), _bell(70, 20) + _bell(20, 5), _bell(50, 30), spike, _bell(30, 25)])
    view = vm.make_view(96, 64, (10, 6, 78, 50), 0.0, 0.5, [10 + 13 * k for k in range(6)], [13] * 6, grid_rows=[16, 36, 55],
                        line_half=1, box_half=2, dot_r2=2)
    return sums, dens, view


def _one():
    """131 x 77, one violin over the whole axes, the axes on the canvas' left edge."""
    sums = np.array([_summary(33, 0.25, 7.75, 0.3)])
    dens = np.stack([_bell(25, 9) + 0.6 * _bell(80, 6)])
    view = vm.make_view(131, 77, (1, 1, 113, 75), -0.5, 0.12, [1], [113], slot_colour=[3], grid_rows=[40, 75], line_half=0, box_half=4,
                        dot_r2=9)
    return sums, dens, view


def _mixed():
    """131 x 77, four violins in slots of unequal width: one without a slot, one without a value, all-equal values."""
    sums = np.array([_summary(40, 1.0, 6.0, 0.2), _summary(30, 2.0, 5.0, 0.2), _summary(0, 0.0, 0.0, 0.0, members=4),
                     _summary(5, 3.25, 3.25, 0.0)])
    dens = np.stack([_bell(50, 15), _bell(50, 15), np.zeros(vm.GRID), np.zeros(vm.GRID)])
    view = vm.make_view(131, 77, (1, 1, 113, 75), 0.0, 0.1, [1, 40, 40, 81], [39, 0, 41, 33], slot_colour=[0, 11, 1, 12], grid_rows=[20],
                        line_half=2, box_half=5, dot_r2=0)
    return sums, dens, view


CASES = {"six": _six, "one": _one, "mixed": _mixed}


@pytest.mark.parametrize("case", sorted(CASES))
def test_profile_and_painter_match_the_model(case):
    from ysmr_amd.plot_functions import device_violins
    sums, dens, view = CASES[case]()
    want = vm.paint_violins(sums, dens, view)
    got = device_violins(sums, dens, vm.to_struct(view), DEV)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    colours = {tuple(p) for p in want.reshape(-1, 3)}
    prof, marks = vm.profile(sums, dens, view)
    if case == "six":
        assert {vm.WHITE, vm.GREY, vm.INNER, vm.BLACK, vm.FILL[0], vm.FILL[2]} <= colours
        assert marks[:, 0].tolist() == [1, 2, 1, 1, 1, 1]
        assert prof[0].max() == 6 and (prof[3] == -1).all() and prof[5].max() == 0 and 0 < (prof[4] >= 1).sum() <= 2
        assert (prof[2][-1] >= 0) and (prof[2][0] == -1)                          # cut by the lower edge of the axes
        assert (want[16, 10:88] == vm.GREY).all(axis=1).any() and not (want[16, 10:88] == vm.GREY).all()   # grid beside and under
    if case == "one":
        assert {vm.WHITE, vm.GREY, vm.INNER, vm.BLACK, vm.FILL[3]} <= colours and (want[1:77, 0] == 0).all()
    if case == "mixed":
        assert {vm.WHITE, vm.GREY, vm.INNER, vm.BLACK, vm.FILL[0]} <= colours and vm.FILL[1] not in colours
        assert marks[:, 0].tolist() == [1, 0, 0, 2] and (want[:, 41:81] != vm.INNER).any(axis=2).all()


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_evaluate_tracks_writes_the_eight_violin_figures(tmp_path):
    import pandas as pd
    from select_tables import select_settings
    from test_gpu_plots import e2e_table
    from ysmr_amd import evaluate_tracks
    from ysmr_amd import plot_functions as pf
    from ysmr_amd.evaluate import violin_cut_list
    df = e2e_table()
    off = select_settings(**{"store generated statistical .csv file": True, "store final analysed .csv file": True,
                             "save large plots": False, "save rose plot": False, "save angle distribution plot / bins": 0})
    on = dict(off, **{"hip violin plots": True})
    os.makedirs(tmp_path / "on")
    os.makedirs(tmp_path / "off")
    out, stats = evaluate_tracks(str(tmp_path / "clip_selected_data.csv"), str(tmp_path / "on"), df=df, settings=on, fps=30.0)
    out_off, stats_off = evaluate_tracks(str(tmp_path / "clip_selected_data.csv"), str(tmp_path / "off"), df=df, settings=off, fps=30.0)
    pd.testing.assert_frame_equal(out, out_off, check_exact=True)
    pd.testing.assert_frame_equal(stats, stats_off, check_exact=True)
    figures = ["Median_speed", "arc-chord_ratio", "displacement", "distance", "perc_motile", "speed", "time_plot", "turning_points"]
    names = sorted(["clip_selected_data_" + n for n in [f + ".png" for f in figures] + ["analysed.csv", "statistics.csv"]])
    assert sorted(os.listdir(tmp_path / "on")) == names
    assert sorted(os.listdir(tmp_path / "off")) == ["clip_selected_data_analysed.csv", "clip_selected_data_statistics.csv"]
    for n in os.listdir(tmp_path / "off"):
        assert (tmp_path / "on" / n).read_bytes() == (tmp_path / "off" / n).read_bytes()
    for f in figures:
        rgb, chunks = png_tools.read_png(str(tmp_path / "on" / ("clip_selected_data_" + f + ".png")))
        assert rgb.shape == (1240, 1753, 3) and chunks[b"pHYs"] == (11811).to_bytes(4, "big") * 2 + b"\x01"

    cut_list = violin_cut_list("Perc. Motile", on["split violin plots on"])
    lo, hi = [a for a, _, _ in cut_list[1:]], [b for _, b, _ in cut_list[1:]]
    for f, column, y_min, y_max in (("speed", "Speed (µm/s)", 0.0, False), ("Median_speed", "Median Speed", None, None)):
        sums, dens = pf.device_violin_stats(stats["Perc. Motile"].to_numpy(), stats[column].to_numpy(), lo, hi, DEV)
        assert sums["members"][0] == len(stats) and (sums["values"] > 0).sum() >= 2
        v, _ = pf.violin_view(sums, y_min, y_max)
        want = vm.paint_violins(sums, dens, vm.from_struct(v))
        rgb, _ = png_tools.read_png(str(tmp_path / "on" / ("clip_selected_data_" + f + ".png")))
        box = np.s_[v.ax_y:v.ax_y + v.ax_h + 1, v.ax_x - 1:v.ax_x + v.ax_w]                       # the axes with their spines
        assert np.array_equal(rgb[box], want[box]), f"{f}: {(rgb[box] != want[box]).any(axis=2).sum()} pixels differ"
        assert (want[box] == vm.FILL[0]).all(axis=2).sum() > 5000 and not np.array_equal(rgb, want)   # violins inside, lettering outside
