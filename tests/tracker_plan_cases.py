"""Which link path a tracker handle takes, shape by shape: one shape on each side of every rule of csrc/tracker_plan.h.

A case is the arguments of ``ysmr_tracker_create`` (DEFAULT with the row's changes), how the gains are made, the handle's
dimensions and link mode, and what is expected:

    path      frame | waves | lanes | batch | batch3 (tracker_plan.h: Link), or error:<which> when creation is refused
    caps      what the configuration qualifies for (tracker_plan.h: Caps), the names in Caps' order
    fused, batched   what ``DeviceTracker.fused`` / ``.batched`` answer.  Recorded from the library of the commit before
              tracker_plan.h existed, on the device, for every row -- not derived from the plan
    further keys     sizes the plan program prints, where a row is about one: frame_lds, batch_lds, batch3_lds (k_batch's
              and k_batch3's with their static part), link_lds

``block`` is the state block's size in bytes, as the commit before carved it (its thirty-five offsets, run stand-alone).

tests/test_tracker_plan_sanitized.py compares all of it with what tests/tracker_plan_check.cc prints, on the CPU;
tests/test_gpu_link.py creates a handle per case (capacity <= 8192) and asks it.

Gains: "closed" = the library's closed form (gains NULL); "cross" = the closed form with a y column of filter 0's x row set
(not decoupled); "bent" = the closed form with the oldest x gain of filter 0 moved (decoupled, not affine in the age);
"faint" = "cross" with a term of 1e-300: not decoupled for the plan, which asks whether the term is zero, while no estimate
changes by a bit (1e-300 times a coordinate is far below half an ulp of the sum it is added to) -- the shape on which the
reference's fixtures reach the wave path with the reference's own three filters.

The ``fixture_*`` rows are the shapes on which tests/test_gpu_batch_link.py runs the operating-point fixtures of
tests/golden/ (FIXTURE has their filter bank); their ``fused`` / ``batched`` follow from the path (they were added after
tracker_plan.h and have no older library to be recorded from).
"""
DEFAULT = dict(max_disappeared=30.0, fps=30.0, n_min=0, n_max=30.0, n_f=3, use_gsff=1, capacity=768, max_det=2048,
               gains="closed", dims=2, link_mode=0)
BIG = dict(capacity=2048, max_det=2500)                   # beyond k_frame: the two-launch paths
D3 = dict(use_gsff=0, dims=3)
FIXTURE = dict(max_disappeared=3.0, fps=12.0, n_max=12.0)  # tests/golden/tracker_{nine,twelve}_waves.npz (crowded_cells: 4.0)

ALL = "frame lanes batch link_lds"
ALL3 = "frame lanes batch batch3 link_lds"

# (name, changes to DEFAULT, path, caps, fused, batched, sizes)
CASES = [
    # the bench's shape and the 4K shape
    ("bench_768_2048", {}, "batch", ALL, False, True, dict(block=1308160, frame_lds=49152, batch_lds=140496)),
    ("bench_768_2048_mode1", dict(link_mode=1), "frame", ALL, True, False, {}),
    ("bench_768_2048_mode2", dict(link_mode=2), "batch", ALL, False, True, {}),
    ("4k_8192_8192", dict(capacity=8192, max_det=8192), "lanes", "lanes link_lds", False, False, dict(block=12782080)),
    # capacity 768 | 769: a track per lane of one workgroup
    ("cap_768", dict(capacity=768), "batch", ALL, False, True, {}),
    ("cap_769", dict(capacity=769), "frame", "frame lanes link_lds", True, False, dict(block=1315072)),
    # max_det 2456 | 2457: the LDS set model
    ("md_2456", dict(max_det=2456), "batch", ALL, False, True, dict(batch_lds=160112)),
    ("md_2457", dict(max_det=2457), "lanes", "lanes link_lds", False, False, {}),
    # k_frame's LDS at 150 KiB
    ("frame_lds_at", dict(capacity=13212, max_det=2456), "frame", "frame lanes link_lds", True, False, dict(frame_lds=153600)),
    ("frame_lds_over", dict(capacity=13213, max_det=2456), "lanes", "lanes link_lds", False, False, dict(frame_lds=153608)),
    # k_batch's LDS at 160 KiB: beyond max_det 2456 already, so the rule cannot decide a path today -- the sizes straddle it
    ("batch_lds_under", dict(max_det=2551), "lanes", "lanes link_lds", False, False, dict(batch_lds=162800)),
    ("batch_lds_over", dict(max_det=2552), "lanes", "lanes link_lds", False, False, dict(batch_lds=164848)),
    # ... and k_batch3's
    ("batch3_lds_under", dict(D3, link_mode=2, max_det=2183), "batch3", ALL3, False, True, dict(batch3_lds=162736)),
    ("batch3_lds_over", dict(D3, link_mode=2, max_det=2184), "frame", ALL, True, False, dict(batch3_lds=164784)),
    # max_disappeared 31999.5 | 32000: k_frame's 15-bit `gone`
    ("gone_31999.5", dict(max_disappeared=31999.5), "batch", ALL, False, True, {}),
    ("gone_32000", dict(max_disappeared=32000.0), "lanes", "lanes link_lds", False, False, {}),
    # n_f 3 | 4: the lane kernels' bank
    ("nf_3", dict(n_f=3), "batch", ALL, False, True, {}),
    ("nf_4", dict(n_f=4), "frame", "frame link_lds", True, False, dict(block=1308672)),
    ("nf_3_big", dict(BIG, n_f=3), "lanes", "lanes link_lds", False, False, {}),
    ("nf_4_big", dict(BIG, n_f=4), "waves", "link_lds", False, False, {}),
    # n_max 31 | 32 (hist_cap 32 | 33: the ring), 63 | 64 (accepted | refused)
    ("nmax_31", dict(n_max=31.0), "batch", ALL, False, True, {}),
    ("nmax_32", dict(n_max=32.0), "frame", "frame link_lds", True, False, {}),
    ("nmax_63", dict(n_max=63.0), "frame", "frame link_lds", True, False, dict(block=1715712)),
    ("nmax_64", dict(n_max=64.0), "error:horizon_max", "", None, None, {}),
    # closed-form gains | caller gains with a cross term | caller gains that are not affine
    ("gains_closed", dict(gains="closed"), "batch", ALL, False, True, {}),
    ("gains_cross", dict(gains="cross"), "frame", "frame link_lds", True, False, {}),
    ("gains_bent", dict(gains="bent"), "frame", "frame link_lds", True, False, {}),
    ("gains_closed_big", dict(BIG, gains="closed"), "lanes", "lanes link_lds", False, False, {}),
    ("gains_cross_big", dict(BIG, gains="cross"), "waves", "link_lds", False, False, {}),
    ("gains_bent_big", dict(BIG, gains="bent"), "waves", "link_lds", False, False, {}),
    # no filter bank
    ("no_gsff", dict(use_gsff=0), "batch", ALL3, False, True, dict(block=888576)),
    # three dimensions, link mode 0 | 1 | 2
    ("d3_mode0", dict(D3, link_mode=0), "frame", ALL3, True, False, {}),
    ("d3_mode1", dict(D3, link_mode=1), "frame", ALL3, True, False, {}),
    ("d3_mode2", dict(D3, link_mode=2), "batch3", ALL3, False, True, dict(batch3_lds=156880)),
    ("d3_mode2_cap_769", dict(D3, link_mode=2, capacity=769), "frame", "frame lanes link_lds", True, False, {}),
    ("d3_mode2_big", dict(D3, link_mode=2, **BIG), "waves", "lanes link_lds", False, False, {}),
    # k_link's tables in LDS: 12 * max_det at 140 KiB
    ("link_lds_at", dict(capacity=1024, max_det=11946), "lanes", "lanes link_lds", False, False, dict(link_lds=143352)),
    ("link_lds_over", dict(capacity=1024, max_det=11947), "lanes", "lanes", False, False, dict(link_lds=143364)),
    # capacity and max_det at 0, 1, 65536 and 65537
    ("cap_0", dict(capacity=0), "error:size", "", None, None, {}),
    ("md_0", dict(max_det=0), "error:size", "", None, None, {}),
    ("cap_1_md_1", dict(capacity=1, max_det=1), "batch", ALL, False, True, dict(block=583680)),
    ("cap_65536", dict(capacity=65536), "lanes", "lanes link_lds", False, False, {}),
    ("md_65536", dict(max_det=65536), "lanes", "lanes", False, False, {}),
    ("cap_65536_md_65536", dict(capacity=65536, max_det=65536), "lanes", "lanes", False, False, dict(block=102238720)),
    ("cap_65537", dict(capacity=65537), "error:size", "", None, None, {}),
    ("md_65537", dict(max_det=65537), "error:size", "", None, None, {}),
    # the operating-point fixtures: one launch per batch, per frame, two per frame with a track per lane / per wave
    ("fixture_batch", dict(FIXTURE), "batch", ALL, False, True, {}),
    ("fixture_frame", dict(FIXTURE, link_mode=1), "frame", ALL, True, False, {}),
    ("fixture_lanes", dict(FIXTURE, **BIG), "lanes", "lanes link_lds", False, False, {}),
    ("fixture_waves", dict(FIXTURE, **BIG, gains="faint"), "waves", "link_lds", False, False, {}),
]
BY_NAME = {c[0]: c for c in CASES}


def arguments(changes):
    """The full arguments of a case."""
    return dict(DEFAULT, **changes)


def perturb_gains(kind, gains):
    """The caller's gains of a case from the closed form (laid out as ``ysmr_gsff_gains`` writes it), in place."""
    if kind == "cross":
        gains[1] = 0.01         # filter 0, x row, the y column of the oldest measurement
    elif kind == "bent":
        gains[0] += 0.01        # filter 0, x row, the x column of the oldest measurement
    elif kind == "faint":
        gains[1] = 1e-300
    return gains


def line_of(name, changes):
    """A case as tracker_plan_check reads it from its standard input."""
    a = arguments(changes)
    return (f"{name} {a['max_disappeared']!r} {a['fps']!r} {a['n_min']} {a['n_max']!r} {a['n_f']} {a['use_gsff']} {a['capacity']} "
            f"{a['max_det']} {a['gains']} {a['dims']} {a['link_mode']}")


def device_tracker(changes):
    """A ``DeviceTracker`` made as the case says (needs the device)."""
    import ctypes

    import numpy as np

    from ysmr_amd import _lib
    from ysmr_amd.tracker import DeviceTracker
    a = arguments(changes)
    gains = None
    if a["gains"] != "closed":
        n_i = (ctypes.c_int32 * a["n_f"])()
        _lib.check(_lib.lib().ysmr_gsff_gains(a["fps"], a["n_min"], a["n_max"], a["n_f"], n_i, None), "ysmr_gsff_gains")
        gains = np.zeros(sum(4 * n for n in n_i))
        _lib.check(_lib.lib().ysmr_gsff_gains(a["fps"], a["n_min"], a["n_max"], a["n_f"], n_i, gains.ctypes.data), "ysmr_gsff_gains")
        perturb_gains(a["gains"], gains)
    return DeviceTracker(max_disappeared=a["max_disappeared"], fps=a["fps"], n_min=a["n_min"], n_max=a["n_max"], n_f=a["n_f"],
                         use_gsff=bool(a["use_gsff"]), capacity=a["capacity"], max_det=a["max_det"], gains=gains,
                         dimensions=a["dims"], link_mode=a["link_mode"])
