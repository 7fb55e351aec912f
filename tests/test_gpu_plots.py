"""GPU: the figure kernels (csrc/plots.hip) against the NumPy model of their rules (plot_model.py), byte for byte, and
the three figures end to end through evaluate_tracks."""
import os

import numpy as np
import pytest

import plot_model as pm
import png_tools

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(DEV)


def _columns(ids, x, y):
    return _dev(ids, np.uint32), _dev(x, np.float64), _dev(y, np.float64)


# ---- extent ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_extent_is_bit_exact(mode):
    from select_tables import make_table
    from ysmr_amd.plot_functions import device_extent
    df = make_table(3, n_tracks=30, max_len=200)
    ids, x, y = df["TRACK_ID"].to_numpy(), df["POSITION_X"].to_numpy().copy(), df["POSITION_Y"].to_numpy().copy()
    x[np.argmax(x)] = np.nan                    # the row with the largest x drops out, with its y
    y[7] = np.inf
    x[len(x) // 2] = -np.inf
    want = pm.extent(ids, x, y, mode, 1.41888781)
    got = device_extent(*_columns(ids, x, y), mode, 1.41888781, DEV)
    assert got.tobytes() == want.tobytes(), (got, want)
    # a first row that is not finite takes its whole track out in mode 1; no row at all
    first = np.flatnonzero(pm.runs(ids)[0])
    x[first[3]] = np.nan
    want = pm.extent(ids, x, y, mode, 0.5)
    assert device_extent(*_columns(ids, x, y), mode, 0.5, DEV).tobytes() == want.tobytes()
    none = device_extent(*_columns(ids[:0], x[:0], y[:0]), mode, 1.0, DEV)
    assert none.tolist() == [np.inf, -np.inf, np.inf, -np.inf]
    nan = device_extent(*_columns(ids[:2], [np.nan, 1.0], [1.0, np.nan]), 0, 1.0, DEV)
    assert nan.tolist() == [np.inf, -np.inf, np.inf, -np.inf]


# ---- the tracks ------------------------------------------------------------------------------------------------------

CANVASES = {"96x64": dict(W=96, H=64, ax=(10, 6, 70, 50), bar=(85, 6, 5, 50), grid_cols=[20, 47, 79], grid_rows=[6, 30]),
            "131x77": dict(W=131, H=77, ax=(1, 1, 113, 75), bar=(120, 3, 9, 71), grid_cols=[1, 57], grid_rows=[40, 75])}
UPP, PX = 0.375, 1.41888781


def _tracks(canvas, mode):
    """(ids, x, y, dist, view): tracks placed by the pixel they are to land on (relative to the axes' corner)."""
    c = CANVASES[canvas]
    w, h = c["ax"][2], c["ax"][3]
    u0, v0 = (-7.0, 3.0) if mode == 0 else (-0.5 * w * UPP, -0.5 * h * UPP)
    rng = np.random.default_rng(w)
    k = np.arange(min(w, h))
    pixel_tracks = [
        np.stack([k, k], 1),                                          # 0, 1: crossing on the same pixels ...
        np.stack([k, k[::-1]], 1),                                    # ... with bit-equal distances
        np.tile([[w // 3, h // 2]], (8, 1)),                          # 2: standing
        np.array([[0, h // 2], [w - 1, h // 3], [w // 2, 0], [w // 4, h - 1], [0, 0], [w - 1, h - 1]]),   # 3: on every edge
        np.array([[-1, 5], [-2, 9], [w, 7], [w + 1, 11], [9, -2], [12, h + 1], [-2, -1], [-3, 20], [w + 40, 5], [5, -700]]),  # 4
        np.stack([rng.integers(-4, w + 4, 40), rng.integers(-4, h + 4, 40)], 1),                           # 5: anywhere
        np.stack([k[: h // 2] + w // 5, np.full(h // 2, h // 2)], 1),  # 6: along a grid row
    ]
    dist = np.array([12.5, 12.5, 0.0, 3.25, 40.0, 7.0, 12.5 * (1 + 2 ** -52)])
    ids, xs, ys = [], [], []
    for t, pix in enumerate(pixel_tracks):
        jitter = rng.uniform(0.05, 0.95, pix.shape)
        u = u0 + (pix[:, 0] + jitter[:, 0]) * UPP
        v = v0 + (pix[:, 1] + jitter[:, 1]) * UPP
        if mode == 1:          # the first row is the track's origin: put one at (0, 0) in front, then move the track
            u, v = np.concatenate([[0.0], u]) + 11.0 * t, np.concatenate([[0.0], v]) - 3.0 * t
        ids.append(np.full(len(u), 5 + 4 * t))
        xs.append(u * PX)
        ys.append(v * PX)
    ids, x, y = np.concatenate(ids), np.concatenate(xs), np.concatenate(ys)
    x[len(k) + 3] = np.nan                                            # a row of track 1
    view = pm.make_view(mode, c["W"], c["H"], c["ax"], u0, v0, UPP, px=PX, grid_cols=c["grid_cols"], grid_rows=c["grid_rows"],
                        bar=c["bar"])
    return ids, x, y, dist, view


def _paint(ids, x, y, dist, view):
    from ysmr_amd.plot_functions import device_tracks
    return device_tracks(*_columns(ids, x, y), dist, pm.to_struct(view), DEV)


@pytest.mark.parametrize("r2_start", [0, 4])
@pytest.mark.parametrize("r2_dot", [0, 1, 5])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("canvas", sorted(CANVASES))
def test_tracks_match_the_model(canvas, mode, r2_dot, r2_start):
    ids, x, y, dist, view = _tracks(canvas, mode)
    view = dict(view, r2_dot=r2_dot, r2_start=r2_start)
    want = pm.paint_tracks(ids, x, y, dist, view)
    got = _paint(ids, x, y, dist, view)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    # the cases are really there: several colours, start dots in mode 0, grid, frame and bar
    colours = {tuple(p) for p in want.reshape(-1, 3)}
    assert len(colours) >= 6 + (mode == 0 and r2_start > 0) and (176, 176, 176) in colours and (0, 0, 0) in colours


@pytest.mark.parametrize("canvas", sorted(CANVASES))
def test_tracks_with_equal_distances_one_row_and_no_row(canvas):
    ids, x, y, dist, view = _tracks(canvas, 0)
    view = dict(view, r2_dot=5)
    for flat in (np.full(len(dist), 3.5), np.where(np.arange(len(dist)) == 2, np.nan, dist)):
        want = pm.paint_tracks(ids, x, y, flat, view)
        assert np.array_equal(_paint(ids, x, y, flat, view), want)
        assert tuple(pm.lut()[0]) in {tuple(p) for p in want.reshape(-1, 3)}          # every track has colour 0
    # the sequential painter itself, once, on the device's input
    assert np.array_equal(_paint(ids, x, y, dist, view), pm.paint_tracks(ids, x, y, dist, view, sequential=True))
    one = (ids[:1], x[:1], y[:1], dist[:1])
    assert np.array_equal(_paint(*one, view), pm.paint_tracks(*one, view))
    empty = (ids[:0], x[:0], y[:0], dist[:0])
    got = _paint(*empty, view)
    assert np.array_equal(got, pm.paint_tracks(*empty, view)) and (got == 255).all(axis=2).sum() > 1000
    # fewer distances than tracks: the tracks beyond them are not drawn
    assert np.array_equal(_paint(ids, x, y, dist[:3], view), pm.paint_tracks(ids, x, y, dist[:3], view))


def test_tracks_grid_stride_loop():
    """200 000 rows in 300 tracks on 640 x 480: more rows than the resident grid has threads.  The rows' track numbers and
    first rows come from csrc/table.h's k_run_flags and k_run_index: this is their stride loop, which the selection and
    the statistics run as well."""
    rng = np.random.default_rng(11)
    lengths = rng.multinomial(200_000 - 300, np.ones(300) / 300) + 1
    ids = np.repeat(np.arange(300, dtype=np.uint32) * 7, lengths)
    start = rng.uniform(0, 600, (300, 2))
    steps = rng.normal(0, 1.2, (len(ids), 2))
    first = np.flatnonzero(pm.runs(ids)[0])
    steps[first] = 0
    walk = np.cumsum(steps, axis=0)
    xy = walk - walk[first][pm.runs(ids)[1]] + start[pm.runs(ids)[1]]
    dist = rng.uniform(0, 300, 300)
    view = pm.make_view(0, 640, 480, (40, 20, 540, 430), -20.0, -30.0, 1.1, px=1.0, r2_dot=1, r2_start=4,
                        grid_cols=[100, 300], grid_rows=[200], bar=(600, 20, 20, 430))
    want = pm.paint_tracks(ids, xy[:, 0], xy[:, 1], dist, view)
    got = _paint(ids, xy[:, 0], xy[:, 1], dist, view)
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    view = dict(view, mode=1, u0=-300.0, v0=-240.0)
    assert np.array_equal(_paint(ids, xy[:, 0], xy[:, 1], dist, view), pm.paint_tracks(ids, xy[:, 0], xy[:, 1], dist, view))


def _walk_columns(lengths):
    from select_tables import walk_table
    df = walk_table(lengths)
    ids = df["TRACK_ID"].to_numpy() * 3 + 2
    dist = np.random.default_rng(len(lengths)).uniform(0, 300, len(lengths))
    return ids, df["POSITION_X"].to_numpy(), df["POSITION_Y"].to_numpy(), dist


WALK_VIEWS = {0: pm.make_view(0, 640, 480, (40, 20, 540, 430), -20.0, -30.0, 1.1, px=1.0, r2_dot=1, r2_start=4, grid_cols=[100, 300],
                              grid_rows=[200], bar=(600, 20, 20, 430))}
WALK_VIEWS[1] = dict(WALK_VIEWS[0], mode=1, u0=-300.0, v0=-240.0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("lengths", ["2047-32-2017-40", "2048-2048-40"])
def test_tracks_starting_at_scan_tile_edges(lengths, mode):
    """Tracks that start on the last row of a scan tile, on the first row of the next and of the third (csrc/table.h:
    index_runs scans in tiles of 2048 rows); with two distances only, the tracks from the third on are not drawn."""
    from select_tables import TILE_EDGE_LENGTHS
    lengths = tuple(int(n) for n in lengths.split("-"))
    assert lengths in TILE_EDGE_LENGTHS
    ids, x, y, dist = _walk_columns(lengths)
    view = WALK_VIEWS[mode]
    want = pm.paint_tracks(ids, x, y, dist, view)
    assert np.array_equal(_paint(ids, x, y, dist, view), want)
    capped = pm.paint_tracks(ids, x, y, dist[:2], view)
    assert np.array_equal(_paint(ids, x, y, dist[:2], view), capped) and not np.array_equal(capped, want)


@pytest.mark.parametrize("mode", [0, 1])
def test_tracks_of_one_row_each(mode):
    """2049 tracks of one row: first[] is used to its full length, past a scan tile."""
    ids, x, y, dist = _walk_columns((1,) * 2049)
    want = pm.paint_tracks(ids, x, y, dist, WALK_VIEWS[mode])
    assert np.array_equal(_paint(ids, x, y, dist, WALK_VIEWS[mode]), want)


# ---- the angle histogram ---------------------------------------------------------------------------------------------

def _histogram(ids, x, y, moving, lag, edges):
    from ysmr_amd.plot_functions import device_angle_histogram
    return device_angle_histogram(*_columns(ids, x, y), _dev(moving, np.int8), lag, edges, DEV)


def histogram_table(seed):
    """A select_tables table with a 'moving' column: per track mostly moving, half and half, or mostly still."""
    from select_tables import make_table
    df = make_table(seed, n_tracks=40, max_len=200)
    rng = np.random.default_rng(100 + seed)
    _, seg, first = pm.runs(df["TRACK_ID"].to_numpy())
    share = rng.choice([0.95, 0.8, 0.72, 0.68, 0.4, 0.0, 1.0], len(first))
    moving = (rng.random(len(df)) < share[seg]).astype(np.int8)
    return df["TRACK_ID"].to_numpy(), df["POSITION_X"].to_numpy(), df["POSITION_Y"].to_numpy(), moving


@pytest.mark.parametrize("n_bins", [36, 7, 1])
@pytest.mark.parametrize("lag", [1, 3])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_histogram_matches_the_model(seed, lag, n_bins):
    ids, x, y, moving = histogram_table(seed)
    edges = np.linspace(-np.pi, np.pi, n_bins + 1)
    # this model's headings are NumPy's arctan2, the device's are correctly rounded (an ulp apart on some arguments): the
    # comparison is only meaningful with every heading clear of the edges (test_histogram_on_lattice_positions: on the edges)
    assert pm.edge_clearance(ids, x, y, moving, lag, edges) > 1e-9
    want, points = pm.angle_histogram(ids, x, y, moving, lag, edges)
    got, got_points = _histogram(ids, x, y, moving, lag, edges)
    assert got_points == points and 0 < want.sum() < points < len(ids)
    assert np.array_equal(got, want), (got, want)


def constructed_histogram_table():
    ids = np.repeat([4, 9, 11, 30], [10, 10, 6, 2])
    moving = np.concatenate([[1] * 7 + [0] * 3,            # 7 of 10: 0.7 > 0.7 is false
                             [1] * 8 + [0] * 2,            # 8 of 10: passes
                             [1] * 6, [1, 1]]).astype(np.int8)
    x = np.concatenate([np.arange(10) * 1.5, np.arange(10) * -0.75 + 0.1 * np.arange(10) ** 2,
                        [5.0, 5.0, 5.0, 5.0, 6.0, 5.0],      # straight up (exact 0), twice down (exact pi), right and back
                        [1.0, 2.0]])
    y = np.concatenate([np.arange(10) * 0.5, np.arange(10) * 1.25,
                        [1.0, 2.0, 1.0, 0.0, 0.3, 0.1],
                        [1.0, 3.0]])
    return ids, x, y, moving


@pytest.mark.parametrize("lag", [1, 3])
def test_histogram_constructed_cases(lag):
    ids, x, y, moving = constructed_histogram_table()
    for n_bins in (36, 8, 2):
        edges = np.linspace(-np.pi, np.pi, n_bins + 1)
        # headings of exactly 0 and pi are here on purpose (dx = 0); every other one is clear of the edges
        assert pm.edge_clearance(ids, x, y, moving, lag, edges, exact=(0.0, np.pi)) > 1e-9
        selected, h = pm.headings(ids, x, y, moving, lag)
        assert selected.tolist() == [False] * 10 + [True] * 8 + [False] * 2 + [True] * 8
        want, points = pm.angle_histogram(ids, x, y, moving, lag, edges)
        assert points == 16 and want.sum() == (13 if lag == 1 else 8)          # the two-row track has no heading at lag 3
        if lag == 1:
            assert (h[selected] == 0.0).sum() == 1 and (h[selected] == np.pi).sum() == 2
        got, got_points = _histogram(ids, x, y, moving, lag, edges)
        assert got_points == points and np.array_equal(got, want), (got, want)
    none = _histogram(ids[:0], x[:0], y[:0], moving[:0], lag, np.linspace(-np.pi, np.pi, 5))
    assert none[1] == 0 and none[0].tolist() == [0, 0, 0, 0]


_LATTICE = {}


def lattice_histogram_table(oracle, seed):
    """A lattice table (select_tables.lattice_table) with the 'moving' column of its own evaluation, built once."""
    if seed not in _LATTICE:
        import warnings
        from atan2_exact import atan2_cr
        from select_tables import lattice_table, select_settings
        df = lattice_table(seed)
        df = df[df.groupby("TRACK_ID")["TRACK_ID"].transform("size") >= 32].reset_index(drop=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rows, _ = oracle.evaluate_tracks_oracle(df, select_settings(), 30.0, arctan2=atan2_cr)
        _LATTICE[seed] = (df["TRACK_ID"].to_numpy(), df["POSITION_X"].to_numpy(), df["POSITION_Y"].to_numpy(),
                          rows["moving"].to_numpy().astype(np.int8))
    return _LATTICE[seed]


@pytest.mark.parametrize("n_bins", [36, 8, 4, 7])
@pytest.mark.parametrize("lag", [1, 3])
def test_histogram_on_lattice_positions(oracle, lag, n_bins):
    """Steps on the 0.5 lattice: the correctly rounded heading of many of them IS an edge of np.linspace(-pi, pi, n + 1)
    (multiples of pi / 4 at 36, 8 and 4 bins; pi alone at 7), and a heading one ulp low falls into the bin before.  No clearance
    here: the counts against the model with correctly rounded headings (tests/atan2_exact.py)."""
    from atan2_exact import atan2_cr
    ids, x, y, moving = lattice_histogram_table(oracle, 1)
    edges = np.linspace(-np.pi, np.pi, n_bins + 1)
    selected, h = pm.headings(ids, x, y, moving, lag, atan2_cr)
    hs = h[selected]
    hs = hs[~np.isnan(hs)]
    on_edge = np.isin(hs, edges)
    print(f"{on_edge.mean():.1%} of {len(hs)} selected headings equal an edge")
    assert len(hs) > 5000 and (on_edge.mean() >= 0.10 if n_bins != 7 else on_edge.sum() >= 1)
    want, points = pm.angle_histogram(ids, x, y, moving, lag, edges, atan2_cr)
    got, got_points = _histogram(ids, x, y, moving, lag, edges)
    assert got_points == points and 0 < want.sum() <= points < len(ids)
    assert np.array_equal(got, want), (got - want)


# ---- the wedges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_bins", [3, 8, 36])
def test_wedges_match_the_model(n_bins):
    from ysmr_amd.plot_functions import device_wedges
    rng = np.random.default_rng(n_bins)
    dirs = pm.wedge_directions(np.linspace(-np.pi, np.pi, n_bins + 1))
    r2 = rng.integers(0, 30 * 30, n_bins)
    r2[rng.integers(0, n_bins)] = 0
    r2[0] = 27 * 27
    for cx, cy, ring_r2 in ((32, 32, 28 * 28), (29, 35, 27 * 27 + 3), (-4, 70, 50 * 50)):
        want = pm.wedges(64, 64, cx, cy, dirs, r2, ring_r2)
        got = device_wedges(64, 64, cx, cy, dirs, r2, ring_r2, DEV)
        assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    colours = {tuple(p) for p in pm.wedges(64, 64, 29, 35, dirs, r2, 27 * 27 + 3).reshape(-1, 3)}
    assert colours == {(255, 255, 255), (0, 0, 0), pm.GRID, pm.BAR_FILL}


# ---- end to end ------------------------------------------------------------------------------------------------------

def e2e_table():
    from select_tables import make_table
    df = make_table(5, n_tracks=25, max_len=500)
    size = df.groupby("TRACK_ID")["TRACK_ID"].transform("size")
    return df[size >= 32].reset_index(drop=True)


def test_evaluate_tracks_writes_the_three_figures(tmp_path):
    import pandas as pd
    from select_tables import select_settings
    from ysmr_amd import evaluate_tracks
    from ysmr_amd import plot_functions as pf
    df = e2e_table()
    on = select_settings(**{"store generated statistical .csv file": True, "store final analysed .csv file": True})
    off = dict(on, **{"save large plots": False, "save rose plot": False, "save angle distribution plot / bins": 0})
    assert on["save large plots"] and on["save rose plot"] and on["save angle distribution plot / bins"] == 36
    os.makedirs(tmp_path / "on")
    os.makedirs(tmp_path / "off")
    out, stats = evaluate_tracks(str(tmp_path / "clip_selected_data.csv"), str(tmp_path / "on"), df=df, settings=on, fps=30.0)
    out_off, stats_off = evaluate_tracks(str(tmp_path / "clip_selected_data.csv"), str(tmp_path / "off"), df=df, settings=off, fps=30.0)
    pd.testing.assert_frame_equal(out, out_off, check_exact=True)
    pd.testing.assert_frame_equal(stats, stats_off, check_exact=True)
    names = ["clip_selected_data_" + n for n in ("Bac_Run_Overview.png", "analysed.csv", "angle_histogram.png", "rose_graph.png",
                                                 "statistics.csv")]
    assert sorted(os.listdir(tmp_path / "on")) == names and sorted(os.listdir(tmp_path / "off")) == [names[1], names[4]]
    for n in (names[1], names[4]):
        assert (tmp_path / "on" / n).read_bytes() == (tmp_path / "off" / n).read_bytes()

    ids, x, y = out["TRACK_ID"].to_numpy(), out["POSITION_X"].to_numpy(), out["POSITION_Y"].to_numpy()
    dist, px = stats["Distance (µm)"].to_numpy(), on["pixel per micrometre"]
    for mode, name in ((0, names[0]), (1, names[3])):
        rgb, chunks = png_tools.read_png(str(tmp_path / "on" / name))
        assert rgb.shape == (2480, 3507, 3) and chunks[b"pHYs"] == (11811).to_bytes(4, "big") * 2 + b"\x01"
        v, _, _ = pf.track_view(pm.extent(ids, x, y, mode, px), mode, px)
        view = pm.make_view(mode, v.width, v.height, (v.ax_x, v.ax_y, v.ax_w, v.ax_h), v.u0, v.v0, v.units_per_pixel, px=px,
                            r2_dot=v.r2_dot, r2_start=v.r2_start, grid_cols=list(v.grid_cols[:v.n_grid_cols]),
                            grid_rows=list(v.grid_rows[:v.n_grid_rows]), bar=(v.bar_x, v.bar_y, v.bar_w, v.bar_h))
        want = pm.paint_tracks(ids, x, y, dist, view)
        box = np.s_[v.ax_y - 1:v.ax_y + v.ax_h + 1, v.ax_x - 1:v.ax_x + v.ax_w + 1]              # the axes with their frame
        assert np.array_equal(rgb[box], want[box]), f"{name}: {(rgb[box] != want[box]).any(axis=2).sum()} pixels differ"
        bar = np.s_[v.bar_y - 1:v.bar_y + v.bar_h + 1, v.bar_x - 1:v.bar_x + v.bar_w + 1]
        assert np.array_equal(rgb[bar], want[bar])
        assert (want[box] != 255).any(axis=2).sum() > 5000 and not np.array_equal(rgb, want)      # tracks inside, lettering outside

    # the angle histogram: the counts from the model (headings clear of the edges), the chart in windows of the canvas
    lag, edges = on["compare angle between n frames"], np.linspace(-np.pi, np.pi, 37)
    moving = out["moving"].to_numpy()
    assert pm.edge_clearance(ids, x, y, moving, lag, edges) > 1e-9
    counts, points = pm.angle_histogram(ids, x, y, moving, lag, edges)
    assert points > 0 and counts.max() > 0
    rgb, _ = png_tools.read_png(str(tmp_path / "on" / names[2]))
    assert rgb.shape == (2480, 3507, 3)
    dirs, bin_of = pf.wedge_boundaries(edges)
    cx, cy, ring_r2, r2 = pf.wedge_plan(counts[bin_of], 3507, 2480)
    ring = int(np.sqrt(ring_r2))
    k = int(np.argmax(counts))
    mid = 0.5 * (edges[k] + edges[k + 1])
    tip = (cx + int(0.9 * ring * np.sin(mid)), cy - int(0.9 * ring * np.cos(mid)))
    rows, cols = np.mgrid[0:2480, 0:3507]
    inside = (cols - cx) ** 2 + (cy - rows) ** 2 <= ring_r2
    for wx, wy in ((cx, cy), tip, (cx, cy - ring + 60), (cx + ring - 60, cy)):                    # centre, longest bar, ring
        x0, y0 = wx - 100, wy - 100
        want = pm.wedges(200, 200, cx - x0, cy - y0, dirs, r2, ring_r2)
        got, disc = rgb[y0:y0 + 200, x0:x0 + 200], inside[y0:y0 + 200, x0:x0 + 200]
        assert np.array_equal(got[disc], want[disc]), f"window at {(wx, wy)}: {(got[disc] != want[disc]).any(axis=1).sum()} pixels differ"
    assert (rgb[inside] == pm.BAR_FILL).all(axis=1).sum() > 10000
