"""GPU: the stages behind the tracker (ysmr_rows_sort, ysmr_rows_format_device, ysmr_select_tracks, ysmr_evaluate_tracks)
at the track and row counts of a real video -- where csrc/prim.h's scan takes its third level (n > 2048 * 2048), the sort by
track for the medians takes two and three radix passes (256 and 65,536 tracks), the resident grids of rows, waves and blocks
start striding (262,144 and 131,072 rows, 1024 tracks), and a track's span no longer fits the reference's uint16.  The
comparisons are those of test_gpu_select.py and test_gpu_evaluate.py, bit for bit; every test first shows, on the oracle's
result alone, that its table lies beyond the size it is named for."""
import numpy as np
import pytest

from select_tables import dust_table, make_table, select_settings, tracker_shaped, value_mix_rows, with_wrapping_spans
from test_gpu_evaluate import _compare as _compare_evaluate, _long_enough
from test_gpu_select import _compare as _compare_select

pytestmark = pytest.mark.gpu

SCAN_3_LEVELS = 2048 * 2048          # csrc/prim.h: SCAN_TILE * SCAN_TILE rows fill two levels exactly
#: the first row that TAKES what the third level computes: tile 2049 adds the scanned tile sum 2048, the first one of the second
#: level's second tile (with 2048 * 2048 + 1 rows the third level runs, and nothing reads its result)
CARRY_3_LEVELS = 2049 * 2048


class _Known:
    """The oracle's answer for one table, worked out once: the size assertions read it, then the comparison does."""

    def __init__(self, *result):
        self.result = result

    def select_tracks_oracle(self, *args):
        return self.result

    def evaluate_tracks_oracle(self, *args):
        return self.result


def _select_oracle(oracle, df, settings):
    return _Known(*oracle.select_tracks_oracle(df, settings, 30.0, 400, 600))


@pytest.mark.parametrize("n_tracks", [255, 256, 257])
def test_select_track_counts_around_one_radix_digit(oracle, n_tracks):
    """255, 256, 257 tracks: the sort by track that serves the area medians goes from one 8-bit pass to two, and the buffer
    that holds its result changes.  The medians are in use: the 'above x times average area' rule drops rows."""
    df = make_table(40 + n_tracks, n_tracks=n_tracks, max_len=120)
    s = select_settings()
    known = _select_oracle(oracle, df, s)
    info = known.result[1]
    assert info["status"] == 0 and info["tracks_before"] == n_tracks and info["good_tracks"] > 0
    assert info["rows_after"] < info["rows_before"]
    _compare_select(known, df, s)


def test_select_more_than_65536_tracks(oracle):
    """48 tracks among 65,600 two-row dust tracks: three radix passes for the medians.  The dust falls to the length rule
    of the clean-up, so what is left is what the 48 tracks give alone."""
    real = make_table(12, n_tracks=48)
    df = dust_table(real, len(real) + 2 * 65600, seed=3)
    s = select_settings()
    alone = oracle.select_tracks_oracle(real, s, 30.0, 400, 600)[1]
    known = _select_oracle(oracle, df, s)
    info = known.result[1]
    assert info["tracks_before"] > 65536 and info["tracks_before"] == 48 + (len(df) - len(real)) // 2
    for k in ("tracks_after", "rows_after", "rows_selected", "good_tracks"):
        assert info[k] == alone[k] > 0, k
    _compare_select(known, df, s)


@pytest.mark.parametrize("n_rows", [SCAN_3_LEVELS + 1, SCAN_3_LEVELS, SCAN_3_LEVELS + 32000],
                         ids=["past-2048x2048", "2048x2048", "selected-track-past-2048x2048"])
def test_select_where_the_scan_takes_three_levels(oracle, n_rows):
    """300 tracks among two million dust tracks, 2048 * 2048 rows and more: the scans behind the track numbers, the first
    and last rows and the places of the compaction carry over a third level.  With the smallest such table (4,194,707 rows)
    the last track lies wholly behind row 2048 * 2048, but it falls to the clean-up and no row takes the third level's
    carry yet (CARRY_3_LEVELS); with 32,000 rows more a track that is SELECTED lies wholly behind row 2049 * 2048, and a
    wrong carry shows in the counts, in its rows and in their index.  And with the front dust of the smallest trimmed to
    2048 * 2048 rows exactly: two levels, both full."""
    df = dust_table(make_table(12, n_tracks=300), max(n_rows, SCAN_3_LEVELS + 1), seed=4)
    assert len(df) > SCAN_3_LEVELS
    if n_rows == SCAN_3_LEVELS:
        df = df.iloc[len(df) - SCAN_3_LEVELS:].reset_index(drop=True)
        assert len(df) == SCAN_3_LEVELS
    s = select_settings()
    known = _select_oracle(oracle, df, s)
    ref, info = known.result
    ids = df["TRACK_ID"].to_numpy()
    assert info["rows_before"] == len(df) >= n_rows and info["tracks_before"] > 2_000_000
    assert info["tracks_after"] > 200 and info["good_tracks"] > 50
    if n_rows > SCAN_3_LEVELS:
        assert ids[SCAN_3_LEVELS - 1] != ids[-1]                                  # the last track: wholly beyond
        if n_rows > SCAN_3_LEVELS + 1:
            start_beyond = set(ids[CARRY_3_LEVELS:]) - {ids[CARRY_3_LEVELS - 1]}
            assert start_beyond & set(ref["TRACK_ID"]), "no selected track lies wholly beyond row 2049 * 2048"
    _compare_select(known, df, s)


@pytest.mark.parametrize("variant", [{}, {"limit track length to x seconds": 0.0, "try to omit motility outliers": False}],
                         ids=["default", "whole-tracks-no-outlier-rule"])
def test_select_past_a_resident_grid_of_rows_and_of_waves(oracle, variant):
    """2700 tracks: more cleaned rows than 1024 blocks of 256 threads hold and more tracks than their 4096 waves."""
    df = make_table(31, n_tracks=2700)
    s = select_settings(**variant)
    known = _select_oracle(oracle, df, s)
    info = known.result[1]
    assert info["rows_after"] > 1024 * 256 and info["tracks_after"] > 1024 and info["good_tracks"] > 100
    assert info["outliers_used"] == (0 if variant else 1) and (bool(variant) or info["dist_outliers"] > 0)
    _compare_select(known, df, s)


def test_select_spans_that_wrap_in_uint16(oracle):
    """Two 2-row tracks whose spans, 65,566 and 65,546 frames, count as 30 and 10 in the reference's uint16: the first is
    kept by the clean-up, the second is dropped."""
    real = make_table(5, n_tracks=20)
    df = with_wrapping_spans(real)
    s = select_settings()
    plain = oracle.select_tracks_oracle(real, s, 30.0, 400, 600)[1]
    known = _select_oracle(oracle, df, s)
    info = known.result[1]
    assert info["rows_after"] == plain["rows_after"] + 2 and info["tracks_after"] == plain["tracks_after"] + 1
    _compare_select(known, df, s)


def test_evaluate_past_1024_tracks_and_131072_rows(oracle):
    """More rows than evaluate's 512 blocks of 256 threads and more tracks than k_ev_tracks has blocks; the row index that
    'df.index // fps' runs through goes up to the table's length."""
    import warnings
    df = _long_enough(make_table(21, n_tracks=1500, max_len=260), 32)
    s, fps = select_settings(), 29.97
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        known = _Known(*oracle.evaluate_tracks_oracle(df, s, fps))
    ref_rows, ref_stats = known.result
    assert len(ref_rows) == len(df) > 512 * 256 and len(ref_stats) > 1024
    assert set(ref_stats["Motility Phenotype"].unique()) == {0, 1, 2}
    _compare_evaluate(known, df, s, fps)


@pytest.mark.parametrize("n", [SCAN_3_LEVELS + 1, CARRY_3_LEVELS + 2 * 2048 + 1], ids=["third-level-runs", "third-level-carries"])
def test_device_formatter_past_2048x2048_rows(n):
    """ysmr_rows_format_device where the scan over the line lengths takes its third level, and where the places of the
    last 4097 lines depend on it; lines of many lengths (a carry that is wrong by a multiple of one length would pass on a
    uniform table): the text byte for byte and the columns bit for bit what the host formatter gives."""
    import torch
    from ysmr_amd import _lib
    from ysmr_amd.helper_file import rows_to_csv_bytes, rows_to_dataframe
    rows = value_mix_rows(n)
    want = np.frombuffer(rows_to_csv_bytes(rows, via_pandas=True), np.uint8)
    ends = np.flatnonzero(want == 10)
    lengths = np.diff(ends)                                   # (the header's line left out)
    assert len(ends) == n + 1 and len(np.unique(lengths)) > 10 and lengths.max() - lengths.min() > 16
    L = _lib.lib()
    dev = torch.from_numpy(rows.view(np.uint8)).cuda()
    cap, ws_bytes = int(L.ysmr_rows_csv_bound(n, 1)), int(L.ysmr_rows_format_device_workspace_bytes(n))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    csv = torch.empty(cap, dtype=torch.uint8, device="cuda")
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")          # csv length; unserved rows (low 32 bits)
    colbuf = torch.empty(48 * n, dtype=torch.uint8, device="cuda")   # TRACK_ID, POSITION_T (uint32), five float64 columns
    base = colbuf.data_ptr()
    _lib.check(L.ysmr_rows_format_device(_lib.stream_ptr(), dev.data_ptr(), n, 1, 1, ws.data_ptr(), ws_bytes, csv.data_ptr(), cap,
                                         meta.data_ptr(), base, base + 4 * n, *[base + 8 * n + 8 * n * k for k in range(5)],
                                         meta[1:].data_ptr()), "ysmr_rows_format_device")
    length, unserved = (int(v) for v in meta.cpu())
    assert unserved & 0xFFFFFFFF == 0
    assert length == len(want)
    got = csv[:length].cpu().numpy()
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, f"{len(differ)} bytes differ, the first at {differ[0]}, in line {np.searchsorted(ends, differ[0])}"
    hc = colbuf.cpu().numpy()
    frame = rows_to_dataframe(rows, via_pandas=True)
    np.testing.assert_array_equal(hc[:4 * n].view(np.uint32), frame["TRACK_ID"].to_numpy())
    np.testing.assert_array_equal(hc[4 * n:8 * n].view(np.uint32), frame["POSITION_T"].to_numpy())
    cols = hc[8 * n:].view(np.uint64).reshape(5, n)
    for k, c in enumerate(("POSITION_X", "POSITION_Y", "WIDTH", "HEIGHT", "DEGREES_ANGLE")):
        np.testing.assert_array_equal(cols[k], frame[c].to_numpy().view(np.uint64), err_msg=c)


def _sort_in_guarded_workspace(rows):
    """ysmr_rows_sort with the workspace and the output carved out of one allocation, guard bands around them -> (sorted
    rows, the workspace's first word: which ordering ran, include/ysmr_hip.h)."""
    import torch
    from ysmr_amd import _lib
    L = _lib.lib()
    GUARD, FILL = 4096, 0xA5
    n, size = len(rows), _lib.ROW_DTYPE.itemsize
    ws_bytes = int(L.ysmr_rows_sort_workspace_bytes(n))
    assert ws_bytes > 0
    off_ws = GUARD
    off_out = (off_ws + ws_bytes + GUARD + 255) // 256 * 256
    total = off_out + n * size + GUARD
    arena = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    dev = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    _lib.check(L.ysmr_rows_sort(_lib.stream_ptr(), dev.data_ptr(), n, arena.data_ptr() + off_ws, ws_bytes,
                                arena.data_ptr() + off_out), "ysmr_rows_sort")
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    inside = np.zeros(total, bool)
    inside[off_ws:off_ws + ws_bytes] = inside[off_out:off_out + n * size] = True
    assert np.all(host[~inside] == FILL), "ysmr_rows_sort wrote outside its workspace or its output"
    return host[off_out:off_out + n * size].view(_lib.ROW_DTYPE), int(host[off_ws:off_ws + 4].view(np.uint32)[0])


@pytest.mark.parametrize("n", [21, 22, 32, 33, 86, 96, 4128, 5000])
def test_rows_sort_serves_the_trackers_table_without_sorting(n):
    """Tables as the link emits them, at row counts on both sides of the sizes at which two buffers of the no-sort path
    once shared bytes of the workspace (n = 22 .. 32, 86 .. 96, 4128: every place then looked taken, and the call fell back
    to the radix sort): the order is right and the call reports the no-sort path."""
    from ysmr_amd import _lib
    rng = np.random.default_rng(n)
    rows = np.zeros(n, _lib.ROW_DTYPE)
    rows["track_id"], rows["frame"] = tracker_shaped(n, 5, seed=n)
    rows["x"], rows["w"] = rng.uniform(0, 1000, n), rng.uniform(0, 10, n).astype(np.float32)
    got, ordering = _sort_in_guarded_workspace(rows)
    assert got.tobytes() == rows[np.lexsort((rows["frame"], rows["track_id"]))].tobytes()
    assert ordering == 0


@pytest.mark.parametrize("n, shape", [(9000, "sparse ids"), (9000, "gaps"), (70001, "duplicates"),
                                      (4000, "a duplicate and a gap that cancel")])
def test_rows_sort_reports_the_radix_sort_for_other_tables(n, shape):
    """The four irregular shapes of test_gpu_pipeline.py::test_rows_sort_on_device: the same word reads 1."""
    from ysmr_amd import _lib
    rng = np.random.default_rng(0)
    rows = np.zeros(n, _lib.ROW_DTYPE)
    perm = rng.permutation(n)
    if shape == "a duplicate and a gap that cancel":
        rows["track_id"], rows["frame"] = perm % 40, perm // 40          # one track's frames: 0, 1, 1, 3, 4, ...
        pick = np.nonzero(rows["track_id"] == 7)[0]
        pick = pick[np.argsort(rows["frame"][pick])]
        rows["frame"][pick[2]] = rows["frame"][pick[1]]
    elif shape == "sparse ids":
        rows["track_id"], rows["frame"] = (perm % 31) * 1_000_003 + 17, perm // 31
    elif shape == "gaps":
        rows["track_id"], rows["frame"] = perm % 31, (perm // 31) * 3 + (perm % 2)
    else:
        rows["track_id"], rows["frame"] = perm % 50, (perm // 50) % 40
    rows["x"] = np.arange(n)
    got, ordering = _sort_in_guarded_workspace(rows)
    assert got.tobytes() == rows[np.lexsort((np.arange(n), rows["frame"], rows["track_id"]))].tobytes()      # stable
    assert ordering == 1
