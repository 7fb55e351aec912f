"""The link-half oracle (oracle/ysmr_oracle.py) pinned against fixtures captured from the
reference's own ysmr/gsff.py and ysmr/tracker.py (tests/golden/gen_golden.py).

The oracle issues the same NumPy/BLAS calls as the reference, so in one environment it is
bit-identical; across machines BLAS/libm may differ in the last bits, hence rtol=1e-12 on floats
and exact equality on every integer quantity (ids, modes, claims, counters).
"""
import numpy as np
import pytest

from conftest import golden, rects_of, tracker_frames

GSFF_CASES = [("gsff_smooth_default.npz", 30.0, 0, 30, 3), ("gsff_jump_default.npz", 30.0, 0, 30, 3),
              ("gsff_turn_default.npz", 30.0, 0, 30, 3), ("gsff_lost_default.npz", 30.0, 0, 30, 3),
              ("gsff_smooth_2997.npz", 29.97, 0, 29.97, 3), ("gsff_jump_nf4.npz", 25.0, 4, 24, 4)]


@pytest.mark.parametrize("name,fps,n_min,n_max,n_f", GSFF_CASES)
def test_gsff_matches_reference(oracle, name, fps, n_min, n_max, n_f):
    g = golden(name)
    f = oracle.OracleGSFF(delta_t=1 / fps, n_min=n_min, n_max=n_max, n_f=n_f)
    assert f.n_i == list(g["n_i"])
    for i, gain in enumerate(f.gains):
        np.testing.assert_allclose(gain, g[f"gain{i}"], rtol=1e-12, atol=1e-15)
    st = oracle.GsffState()
    for k, z in enumerate(g["fed"]):
        c = f.correct(np.array(z), st)
        p = f.predict(st)
        assert st.mode == g["mode"][k]
        np.testing.assert_allclose(c, g["correct"][k], rtol=1e-12)
        np.testing.assert_allclose(p, g["predict"][k], rtol=1e-12)
        np.testing.assert_allclose(st.weights, g["weights"][k][:st.mode], rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(st.likelihoods, g["likelihoods"][k][:st.mode], rtol=1e-10, atol=1e-300)


def test_gsff_horizons_and_closed_form(oracle):
    assert oracle.horizon_sizes(0, 30, 3) == [10, 20, 30]
    assert oracle.horizon_sizes(0, 29.97, 3) == [9, 19, 29]
    # rows 0/1 of the gain are decoupled and equal the one-step-ahead LS line-fit predictor
    for n in (9, 10, 20, 30):
        gain = oracle.lsf_gain(n, 1 / 30.0)
        t = np.arange(n) - (n - 1) / 2
        coef = 1 / n + t * ((n + 1) / 2) / np.sum(t * t)
        np.testing.assert_allclose(gain[0, 0::2], coef, atol=1e-12)
        np.testing.assert_allclose(gain[1, 1::2], coef, atol=1e-12)
        assert np.all(gain[0, 1::2] == 0) and np.all(gain[1, 0::2] == 0)


TRACKER_CASES = ["tracker_small_gsff.npz", "tracker_small_nogsff.npz", "tracker_mid_gsff.npz",
                 "tracker_gap.npz", "tracker_2997.npz",
                 "tracker_nine_waves.npz", "tracker_twelve_waves.npz", "tracker_crowded_cells.npz"]


@pytest.mark.parametrize("name", TRACKER_CASES)
def test_tracker_matches_reference(oracle, name):
    g = golden(name)
    fps = float(g["fps"])
    n_max = None if int(g["n_max"]) < 0 else int(g["n_max"])
    max_gone = float(g["max_disappeared"]) if "max_disappeared" in g.files else {"tracker_gap.npz": 5, "tracker_2997.npz": 6}.get(name, fps)
    tr = oracle.OracleTracker(max_disappeared=max_gone, fps=fps, n_min=int(g["n_min"]), n_max=n_max,
                              n_f=int(g["n_f"]), use_gsff=bool(g["use_gsff"]))
    off, coff = g["off"], g["claim_off"]
    for f, (det, info) in enumerate(tracker_frames(g)):
        ids, xy, inf, claims = tr.update(rects_of(det, info))
        sl = slice(off[f], off[f + 1])
        assert ids == list(g["ids"][sl]), f"frame {f}"
        np.testing.assert_allclose(xy, g["xy"][sl], rtol=1e-12, err_msg=f"frame {f}")
        np.testing.assert_array_equal(np.array([list(i) for i in inf], dtype=float).reshape(-1, 3), g["info"][sl])
        assert [t.gone for t in tr.tracks] == list(g["disappeared"][sl])
        assert tr.next_id == g["next_id"][f]
        assert sorted(claims) == sorted(map(tuple, g["claims"][coff[f]:coff[f + 1]].tolist())), f"frame {f}"



def test_batch_link_clips_reach_the_states_their_gpu_tests_are_about(oracle):
    """tests/link_clips.py builds the detection sequences of the batch link's GPU tests at the states where k_batch's code
    paths change: more than 704 live tracks for >= 70 frames with deaths and births in that state (all
    twelve waves seated), frames of more than 600 detections (48 cells per side, the wave search without its float
    pre-pass).  Checked here, on the CPU, so that an edit of a generator cannot quietly move a test off its path."""
    from link_clips import crowded_clip, dense_detection_clip, oracle_rows
    kw = dict(max_disappeared=5.0, fps=30.0, n_min=0, n_max=30, n_f=3)
    frames = crowded_clip()
    rows, live, ot = oracle_rows(oracle, frames, use_gsff=True, **kw)
    assert len(frames) >= 100 and live.min() >= 716 and live.max() <= 768           # seats 705.. of the twelfth wave in use throughout
    assert ot.next_id - live[-1] >= 60                                               # deaths ...
    births = [f for f in range(1, len(live)) if max(r[1] for r in rows if r[0] == f) > max(r[1] for r in rows if r[0] == f - 1)]
    assert len(births) >= 5 and all(live[f - 1] >= 716 for f in births)             # ... and births in that state
    assert any(32 < f < 96 for f in births)
    for stationary in (False, True):
        frames = dense_detection_clip(stationary=stationary)
        rows, live, ot = oracle_rows(oracle, frames, use_gsff=not stationary, **kw)
        m = np.array([len(d) for d, _ in frames])
        assert live.max() <= 768 and live.min() > 704 and m.min() > 600 and m.max() <= 768


# name: (live tracks: more than, at most), (detections per frame: more than, at most) -- tests/golden/gen_golden.py: OPERATING_POINT
OPERATING_POINT = {"tracker_nine_waves.npz": ((512, 576), (128, 600)), "tracker_twelve_waves.npz": ((704, 768), (600, 768)),
                   "tracker_crowded_cells.npz": ((299, 500), (128, 600))}


@pytest.mark.parametrize("name", list(OPERATING_POINT))
def test_operating_point_fixtures_hold_the_states_their_gpu_tests_are_about(name):
    """The three fixtures that pin the link to the reference at its operating point, from the committed files alone: live
    tracks (nine waves: 513 .. 576, twelve: 705 .. 768) and detections (twelve waves: more than 600, i.e. 48 cells per side
    and no candidate lists) in EVERY frame, at least 20 ids issued after frame 0, at least 20 tracks deregistered, at least
    ten frames after the first in which a track has its third filter (a track of frame 0 that was never dropped has
    n_i[2] = n_max measurements in its window from frame n_max - n_i[0] on), and for the crowded clip, by the model of
    k_bgrid's lists (tests/cell_list_model.py), a split cell in at least half of the frames and a cell that stays flagged
    (the 3 x 3 search) in at least one.  A regenerated fixture cannot quietly move a GPU test off its path."""
    import cell_list_model as cm
    g = golden(name)
    (live_above, live_most), (det_above, det_most) = OPERATING_POINT[name]
    live, m = np.diff(g["off"]), np.diff(g["det_off"])
    assert live.min() > live_above and live.max() <= live_most, (live.min(), live.max())
    assert m.min() > det_above and m.max() <= det_most, (m.min(), m.max())
    assert bool(g["use_gsff"]) and int(g["n_f"]) == 3 and int(g["n_min"]) == 0 and 3 <= float(g["max_disappeared"]) <= 5
    assert g["det_info"].dtype == np.float32 and g["info"].dtype == np.float32
    assert np.array_equal(g["det"], g["det"].astype(np.float32).astype(np.float64))       # what the device is handed
    next_id = g["next_id"]
    assert next_id[0] == live[0] and next_id[-1] - next_id[0] >= 20                        # births after frame 0
    assert next_id[-1] - live[-1] >= 20                                                    # deaths
    n_max = int(g["n_max"])
    first_full_bank = n_max - n_max // 3
    ids = [set(g["ids"][g["off"][f]:g["off"][f + 1]].tolist()) for f in range(len(live))]
    assert set.intersection(*ids[:first_full_bank + 1]) and len(live) - 1 - first_full_bank >= 10
    if name == "tracker_crowded_cells.npz":
        split = flagged = 0
        for det, _ in tracker_frames(g):
            grid, order = cm.bin_frame(det)
            assert cm.has_lists(len(det))
            lists, _ = cm.frame_lists(grid, det.astype(np.float32)[order])
            split += bool((lists[:, 0] == cm.SPLIT).any())
            flagged += bool((lists[:, 0] == cm.FLAG).any())
        assert 2 * split >= len(live) and flagged >= 1, (split, flagged)
