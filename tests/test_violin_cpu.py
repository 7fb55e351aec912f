"""CPU: the NumPy model of the violin plots (violin_model.py) against scipy, NumPy and pandas, the cut list of
evaluate_tracks, and the wiring of 'hip violin plots' with the device calls stubbed."""
import logging
import os

import numpy as np
import pytest

import png_tools
import violin_model as vm
from test_plots_cpu import OFF, _run, _settings, _stub_device

SIZES = (2, 3, 17, 257, 4096)


def _data(kind, n):
    rng = np.random.default_rng(1000 + n)
    return rng.gamma(2.0, 3.0, n) if kind == "gamma" else np.round(rng.uniform(0.0, 12.0, n), 1)


# ---- the model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["gamma", "uniform"])
def test_model_density_is_scipys_gaussian_kde(kind, n):
    """seaborn's violinplot(cut=0, bw=.2, gridsize=100) evaluates scipy.stats.gaussian_kde(x, bw_method=0.2) on
    linspace(min, max, 100).  Well-spread data only: on tightly clustered values scipy's own whitening loses digits the
    formula keeps."""
    from scipy.stats import gaussian_kde
    x = np.sort(_data(kind, n))
    assert x[0] < x[-1]
    s = vm.summary(n, x)
    grid = vm.grid_points(s["vmin"], s["vmax"])
    assert np.array_equal(grid, np.linspace(x[0], x[-1], vm.GRID))
    assert s["h"] == pytest.approx(0.2 * np.std(x, ddof=1), rel=1e-14)
    want = gaussian_kde(x, bw_method=0.2).evaluate(grid)
    got = vm.density(x, s)
    worst = np.abs(got - want).max() / want.max()
    print(kind, n, "worst error / peak", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("n", (1,) + SIZES)
@pytest.mark.parametrize("kind", ["gamma", "uniform"])
def test_model_summaries_are_numpys_and_pandas(kind, n):
    import pandas as pd
    x = np.sort(_data(kind, n))
    s = vm.summary(n + 2, x)
    want = np.percentile(x, [25, 50, 75])
    assert np.array([s["q25"], s["q50"], s["q75"]]).tobytes() == want.tobytes()
    series = pd.Series(x)
    assert s["q50"] == series.median()
    # any order of adding n positive numbers is within (n - 1) 2^-53 of their sum, fsum within 2^-53
    assert abs(s["mean"] - series.mean()) <= n * 2.0 ** -53 * s["mean"]
    assert (s["members"], s["values"], s["vmin"], s["vmax"]) == (n + 2, n, x[0], x[-1])
    iqr = want[2] - want[0]
    assert s["whisker_lo"] == x[x >= want[0] - 1.5 * iqr].min() and s["whisker_hi"] == x[x <= want[2] + 1.5 * iqr].max()


def test_model_categories_follow_upstreams_loop():
    """np.where over the cut list in order, later intervals overwriting earlier ones (track_eval.py:1188-1198)."""
    rng = np.random.default_rng(2)
    cut = np.concatenate([rng.uniform(-10, 110, 500), [0.0, 20.0, 100.01, np.nan, np.inf]])
    for lo, hi in (([0.0, 20.0, 40.0], [20.0, 40.0, 100.01]), ([0.0, 10.0, 5.0, 50.0], [30.0, 20.0, 15.0, 40.0])):
        want = np.full(len(cut), np.nan)
        with np.errstate(invalid="ignore"):
            for k, (a, b) in enumerate(zip(lo, hi)):
                want = np.where((a <= cut) & (b > cut), k + 1, want)
        got = vm.categories(cut, lo, hi)
        assert np.array_equal(got, np.nan_to_num(want, nan=0.0).astype(np.int64))
        groups = vm.violin_values(cut, cut, lo, hi)
        assert groups[0][0] == len(cut) and len(groups[0][1]) == len(cut) - 2       # 'All': every track; finite values only
        assert [g[0] for g in groups[1:]] == [(got == k + 1).sum() for k in range(len(lo))]


# ---- the cut list ----------------------------------------------------------------------------------------------------

def test_cut_list_has_upstreams_three_label_forms():
    from ysmr_amd.evaluate import violin_cut_list
    splits = [0.0, 20.0, 40.0, 60.0, 80.0, 100.01]
    assert violin_cut_list("Perc. Motile", splits) == [(-np.inf, np.inf, "All"), (0.0, 20.0, "0.0% - 20.0%"), (20.0, 40.0, "20.0% - 40.0%"),
                                                     (40.0, 60.0, "40.0% - 60.0%"), (60.0, 80.0, "60.0% - 80.0%"),
                                                     (80.0, 100.01, "80.0% - 100.0%")]
    assert violin_cut_list("Motility Phenotype", splits) == [(-np.inf, np.inf, "All"), (0, 0.001, "Immotile"), (1, 1.001, "Twitching"),
                                                           (2, 2.001, "Motile")]
    assert violin_cut_list("Speed (µm/s)", [0.0, 2.5, 10.0]) == [(-np.inf, np.inf, "All"), (0.0, 2.5, "0.00 - 2.50"), (2.5, 10.0, "2.50 - 10.00")]
    # an overlapping, non-monotone list: consecutive pairs as they come, empty intervals included
    assert violin_cut_list("Time (s)", [0.0, 30.0, 10.0, 20.0, 5.0])[1:] == [(0.0, 30.0, "0.00 - 30.00"), (30.0, 10.0, "30.00 - 10.00"),
                                                                            (10.0, 20.0, "10.00 - 20.00"), (20.0, 5.0, "20.00 - 5.00")]
    assert violin_cut_list("Time (s)", [1.0]) == [(-np.inf, np.inf, "All")]


# ---- the wiring ------------------------------------------------------------------------------------------------------

VIOLIN_KEYS = {"save turning point violin plot": "turning_points", "save length violin plot": "distance", "save speed violin plot": "speed",
               "save time violin plot": "time_plot", "save displacement violin plot": "displacement",
               "save percent motile plot": "perc_motile", "save acr violin plot": "arc-chord_ratio"}
NO_VIOLINS = {k: False for k in VIOLIN_KEYS}
PREFIX = "210102030405_clip_selected_data_"


def _stub_violins(monkeypatch, calls, fail=None):
    from ysmr_amd import plot_functions as pf
    _stub_device(monkeypatch, [])

    def stats(cut, value, lo, hi, dev):
        calls.append(("stats", len(cut), list(lo), list(hi)))
        return vm.stats(cut, value, lo, hi)

    def violins(sums, dens, view, dev):
        if fail is not None and len(calls) // 2 == fail:
            raise RuntimeError("no violin today")
        calls.append(("violins", view.n_violins, view.width, view.height))
        return np.full((view.height, view.width, 3), 255, np.uint8)

    monkeypatch.setattr(pf, "device_violin_stats", stats)
    monkeypatch.setattr(pf, "device_violins", violins)


def _csv(files):
    return {k: v for k, v in files.items() if k.endswith(".csv")}


def test_without_the_key_nothing_changes(tmp_path, monkeypatch, caplog):
    caplog.set_level(logging.INFO, logger="ysmr")
    calls = []
    _stub_violins(monkeypatch, calls)
    for name, extra in (("absent", {}), ("false", {"hip violin plots": False})):
        caplog.clear()
        _, files = _run(tmp_path, name, _settings(**dict(OFF, **extra)))
        assert sorted(files) == [PREFIX + "analysed.csv", PREFIX + "statistics.csv"] and calls == []
        assert "Plots are not part of the HIP path; skipped: save time violin plot" in caplog.text


def test_with_the_key_the_figures_the_settings_ask_for_are_written(tmp_path, monkeypatch, caplog):
    from ysmr_amd import plot_functions as pf
    caplog.set_level(logging.INFO, logger="ysmr")
    calls = []
    _stub_violins(monkeypatch, calls)
    (df_off, stats_off), files_off = _run(tmp_path, "off", _settings(**OFF))
    caplog.clear()
    on = dict(OFF, **{"hip violin plots": True})
    (df_on, stats_on), files_on = _run(tmp_path, "on", _settings(**on))
    assert "skipped" not in caplog.text and "failed" not in caplog.text
    everything = sorted(VIOLIN_KEYS.values()) + ["Median_speed"]
    assert sorted(files_on) == sorted([PREFIX + n + ".png" for n in everything] + list(files_off))
    assert df_on.equals(df_off) and stats_on.equals(stats_off) and _csv(files_on) == files_off
    assert list(stats_on.columns)[-1] == "Categories (Perc. Motile)" and (stats_on.iloc[:, -1] == "All").all()
    # upstream's order, two device calls a figure; the default split: five intervals beside 'All', four tracks
    assert [c[0] for c in calls] == ["stats", "violins"] * 8
    assert calls[0] == ("stats", 4, [0.0, 20.0, 40.0, 60.0, 80.0], [20.0, 40.0, 60.0, 80.0, 100.01]) and calls[1] == ("violins", 6, 1753, 1240)
    rgb, chunks = png_tools.read_png(str(tmp_path / "on" / (PREFIX + "distance.png")))
    assert rgb.shape == (1240, 1753, 3) and chunks[b"pHYs"][:4] == (11811).to_bytes(4, "big")
    x, y, w, h = pf.violin_layout(1753, 1240)
    assert (rgb[y:y + h, x:x + w] == 255).all()                                  # lettering stays outside the axes
    ink = (rgb == 0).all(axis=2)
    assert ink[:y - 60].any() and ink[y - 60:y].any() and ink[y + h:].any() and ink[y:y + h, :x].any()   # title, boxes, names, ticks
    # one key at a time, and none: Median_speed is drawn always
    for key, name in VIOLIN_KEYS.items():
        _, files = _run(tmp_path, name[:6], _settings(**dict(on, **dict(NO_VIOLINS, **{key: True}))))
        assert sorted(files) == sorted([PREFIX + name + ".png", PREFIX + "Median_speed.png"] + list(files_off))
        assert _csv(files) == files_off
    _, files = _run(tmp_path, "none", _settings(**dict(on, **NO_VIOLINS)))
    assert sorted(files) == sorted([PREFIX + "Median_speed.png"] + list(files_off)) and _csv(files) == files_off
    # beside the track figures
    _, files = _run(tmp_path, "all", _settings(**{"hip violin plots": True}))
    tracks = ["Bac_Run_Overview", "angle_histogram", "rose_graph"]
    assert sorted(files) == sorted([PREFIX + n + ".png" for n in everything + tracks] + list(files_off)) and _csv(files) == files_off


def test_other_splits_and_a_failing_figure(tmp_path, monkeypatch, caplog):
    calls = []
    _stub_violins(monkeypatch, calls)
    key = "split results by (Turn Points / Distance / Speed / Time / Displacement / perc. motile)"
    on = dict(OFF, **dict(NO_VIOLINS, **{"hip violin plots": True}))
    (df_ref, stats_ref), files_ref = _run(tmp_path, "ref", _settings(**dict(OFF, **{key: "Distance"})))
    (df, stats), files = _run(tmp_path, "dist", _settings(**dict(on, **{key: "Distance", "split violin plots on": [0.0, 7.5, 6.5, 100.0]})))
    assert calls[0] == ("stats", 4, [0.0, 7.5, 6.5], [7.5, 6.5, 100.0]) and calls[1] == ("violins", 4, 1753, 1240)
    assert df.equals(df_ref) and stats.equals(stats_ref) and _csv(files) == files_ref
    calls.clear()
    _run(tmp_path, "phen", _settings(**dict(on, **{key: "Phenotype"})))
    assert calls[0] == ("stats", 4, [0.0, 1.0, 2.0], [0.001, 1.001, 2.001])
    # the second of three figures fails: an error in the log, the others and the tables are there
    calls.clear()
    _stub_violins(monkeypatch, calls, fail=1)
    (df, stats), files = _run(tmp_path, "fail", _settings(**dict(on, **{key: "Distance", "save length violin plot": True,
                                                                        "save speed violin plot": True})))
    assert sorted(files) == sorted([PREFIX + "distance.png", PREFIX + "Median_speed.png"] + list(files_ref))
    assert caplog.text.count("no violin today") == 1 and "speed.png failed" in caplog.text
    assert df.equals(df_ref) and _csv(files) == files_ref


def test_violin_plot_limits_and_missing_categories(tmp_path, monkeypatch):
    """False or None for a limit is automatic; a category without a value gets no slot and no text box."""
    import pandas as pd
    from ysmr_amd import plot_functions as pf
    cut = np.array([5.0, 5.0, 30.0, 30.0, 30.0, 90.0, np.nan])
    value = np.array([1.0, 3.0, 2.0, 4.0, 6.0, np.nan, 11.0])
    sums, _ = vm.stats(cut, value, [0.0, 20.0, 40.0, 80.0], [20.0, 40.0, 80.0, 100.01])
    labels = ["All", "a", "b", "c", "d"]
    boxes = pf.violin_text_boxes(sums, labels)
    assert [v for v, _ in boxes] == [0, 1, 2]
    assert boxes[1][1] == "a: 2 (28.6%)\nMedian: 2.00\nAverage:  2.00" and boxes[0][1].startswith("All: 7 (100.0%)\nMedian: 3.50")
    view, rows = pf.violin_view(sums, False, None)
    assert view.y0 == 1.0 - 0.5 and view.y0 + view.units_per_pixel * view.ax_h == pytest.approx(11.5)
    assert [view.slot_w[v] > 0 for v in range(5)] == [True, True, True, False, False]
    assert view.slot_x[0] == view.ax_x and view.slot_x[2] + view.slot_w[2] == view.ax_x + view.ax_w
    assert [view.slot_colour[v] for v in range(3)] == [0, 1, 2]
    assert len(rows) == view.n_grid_rows > 2 and all(view.ax_y <= r < view.ax_y + view.ax_h for _, r in rows)
    view, _ = pf.violin_view(sums, 0.0, 100.0)
    assert view.y0 == 0.0 and view.units_per_pixel == 100.0 / view.ax_h
    with pytest.raises(ValueError):
        pf.violin_view(np.zeros(65, vm.SUMMARY_DTYPE))
    with pytest.raises(ValueError):
        pf.violin_plot(pd.DataFrame({"a": [1.0]}), str(tmp_path / "x.png"), "a", "Groups", [(-np.inf, np.inf, "All")], device="cpu")
    assert not os.listdir(tmp_path)
